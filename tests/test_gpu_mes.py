"""GPU (-m gpu): gpbo_mes_argbest — max-value entropy search values over the resident candidates and their selection — against
tests/mes_truth.py, and suggest_mes on the real engine.

Values.  The device's own mu / sd are fetched, y* is built from them so that gamma = (y* - mu) / sd covers every range of h — the
lower tail on both sides of the series switch at -28, both sides of -1, 0, the complement branch up to gamma = 36 where h ~ 1e-281 —
and ys_out is compared with the truth ON THOSE mu / sd: `mes_values` (held to the 60-digit truth at 5.7e-14 in
tests/test_mes_host.py) for every candidate, the 60-digit truth itself at the targeted candidates.  Bar: 1e-9 relative (values below
1e-290: 1e-299 absolute), the project's bar; the (1 + gamma^2) eps model of the division that makes gamma is at most 3e-13 here.
Selection: exact against the returned ys_out; against the truth where the truth's own top k + 1 are further apart than the bar
(asserted on the truth alone).  Shapes: N = 40, d = 3 and N = 300, d = 17; M = 1000 and M = 257, both ragged against the 256-thread
block, M = 257 two blocks with one live thread in the second.

Conventions, the reader contract (tests/test_gpu_call_order.py's sense: the call is invisible to every later call), the refusals,
and suggest_mes end to end over a driver built the way accelerate() leaves a BayesianOptimization."""
import functools

import numpy as np
import pytest

import batch_truth as B
import matern_family_truth as F
import mes_truth as T
from bayesianoptimization_amd import _lib
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd import suggest_mes
from bayesianoptimization_amd._lib import GpboError, dptr, iptr
from bayesianoptimization_amd.engine import GpEngine, GroupEngine
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

NOISE = 1e-4
Y_MEAN, Y_STD = 3.5, 0.4
TARGETS = (-40.0, -28.5, -27.5, -5.0, -1.001, -0.999, 0.0, 0.5, 6.0, 15.0, 36.0)
#: name -> (N, d, M, kind)
CASES = {"n40-d3-m1000": (40, 3, 1000, F.MATERN25), "n40-d3-m257": (40, 3, 257, F.MATERN25), "n300-d17-m1000": (300, 17, 1000, F.RBF)}


class Case:
    """Data of one case (computed once, shared, never changed); the posterior is the device's own, fetched per test."""

    def __init__(self, N, d, M, kind):
        self.N, self.d, self.M, self.kind = N, d, M, kind
        self.X, y = F.data(N, d, seed=3 * N + d)
        self.yn = (y - y.mean()) / y.std()
        self.ls = 0.5 * np.sqrt(d) * np.geomspace(0.75, 1.33, d)
        self.Xc = np.random.RandomState(500 + N + d).uniform(size=(1000, d))[:M]      # M = 257: the first rows of M = 1000
        self.rows = (37 * np.arange(len(TARGETS)) + 5) % M                              # the candidate each target gamma is aimed at
        self.what = f"N={N} d={d} M={M}"

    def posterior(self, eng, Xc=None):
        eng.fit(self.X, self.yn, self.kind, self.ls, NOISE)
        eng.set_candidates(self.Xc if Xc is None else Xc)
        return eng.posterior(0, Y_MEAN, Y_STD)

    def y_star(self, mu, sd, S):
        """S sampled maxima: the targets first (S = 5: every other one), the rest spread over the posterior's own range"""
        aimed = mu[self.rows] + np.array(TARGETS) * sd[self.rows]
        aimed = aimed[::2][:S] if S < len(TARGETS) else aimed
        rs = np.random.RandomState(S)
        rest = rs.uniform(mu.min() - 3 * sd.max(), mu.max() + 3 * sd.max(), size=S - aimed.shape[0])
        return np.concatenate([aimed, rest])


@functools.lru_cache(maxsize=None)
def case_of(name):
    return Case(*CASES[name])


def check_values(what, ys, mu, sd, y_star):
    want = -T.mes_values(mu, sd, y_star)
    worst, ok = T.within_bar(ys, want)
    print(f"{what} S={len(y_star)}: worst error / max(|truth|, 1e-290) = {worst:.2e} (bar {T.BAR:.0e})")
    assert ok, f"{what} S={len(y_star)}: {worst:.2e} over the bar"
    assert (ys[~np.isnan(ys)] <= 0).all()
    return worst


# ---- values ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_values_over_every_range(engine, name):
    c = case_of(name)
    mu, sd = c.posterior(engine)
    assert (sd > 0).all() and np.isfinite(mu).all()
    # one sample at a time: each target gamma alone, so that the tails are not summed away — and the 60-digit truth at its candidate
    for t, (row, target) in enumerate(zip(c.rows, TARGETS)):
        y = mu[row] + target * sd[row]
        bi, bv, si, sv, ys = engine.mes_argbest([y], return_values=True)
        assert ys.shape == (c.M,)
        check_values(f"{c.what} gamma={target}", ys, mu, sd, [y])
        g = T.gamma_mp(y, mu[row], sd[row])
        truth = float(T.h_truth(g))
        assert abs(float(g) - target) <= 1e-6 * max(1.0, abs(target)), "the construction missed its target"
        err = abs(-ys[row] - truth) / max(truth, T.TINY)
        print(f"{c.what} gamma={float(g)!r}: device {-ys[row]!r} truth {truth!r} error {err:.2e}")
        assert err <= T.BAR
    for S in (5, 16, 64):
        y_star = c.y_star(mu, sd, S)
        bi, bv, si, sv, ys = engine.mes_argbest(y_star, return_values=True)
        check_values(c.what, ys, mu, sd, y_star)
        assert bi == int(np.argmin(ys)) and bv == ys[bi]


# ---- selection -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n40-d3-m1000", "n40-d3-m257"])
def test_selection(engine, name):
    c = case_of(name)
    mu, sd = c.posterior(engine)
    y_star = c.y_star(mu, sd, 16)
    truth = T.mes_values(mu, sd, y_star)
    for k in (0, 1, 2, 3, 16, 64):          # one or two picks: the pass form; from three on: threshold + ranks
        bi, bv, si, sv, ys = engine.mes_argbest(y_star, k_seeds=k, return_values=True)
        # exactly the argmin / stable argsort[:k] of the values the call itself returned
        wi, wv, wsi, wsv = T.argbest(ys, k)
        assert bi == wi and bv == wv and np.array_equal(si, wsi) and np.array_equal(sv, wsv), (c.what, k)
        assert si.shape == (k,) and sv.shape == (k,)
        # ... and the truth's ranking, where the truth alone separates its top k + 1 by more than the bar
        assert T.separated_top(truth, max(k, 1)), f"{c.what}: the truth's own top {k + 1} are within the bar: pick another seed"
        order = np.argsort(-truth, kind="stable")
        assert bi == int(order[0]) and np.array_equal(si, order[:k]), (c.what, k)
        # index_offset shifts every returned index and nothing else
        oi, ov, osi, osv, _ = engine.mes_argbest(y_star, k_seeds=k, index_offset=10**10)
        assert oi == bi + 10**10 and ov == bv and np.array_equal(osi, si + 10**10) and np.array_equal(osv, sv)


def test_fewer_candidates_than_seeds(engine):
    c = case_of("n40-d3-m257")
    mu, sd = c.posterior(engine, c.Xc[:5])
    bi, bv, si, sv, ys = engine.mes_argbest([float(mu.max() + sd.max())], k_seeds=8, return_values=True)
    wi, wv, wsi, wsv = T.argbest(ys, 5)
    assert ys.shape == (5,) and bi == wi and np.array_equal(si[:5], wsi) and np.array_equal(sv[:5], wsv)
    assert (si[5:] == -1).all()


# ---- conventions -----------------------------------------------------------------------------------------------------------------
def test_one_sample_orders_by_minus_gamma(engine):
    c = case_of("n40-d3-m1000")
    mu, sd = c.posterior(engine)
    y = float(np.quantile(mu, 0.9))
    g = (y - mu) / sd
    assert g.min() < -1.0 and (g > 0).sum() > 100 and g.max() > 40.0      # all three ranges, and the zeros above gamma = 40
    bi, bv, si, sv, ys = engine.mes_argbest([y], k_seeds=32, return_values=True)
    order = np.argsort(g, kind="stable")
    assert T.separated_top(T.mes_values(mu, sd, [y]), 32)
    assert bi == int(order[0]) and np.array_equal(si, order[:32])
    along = ys[order]                       # non-decreasing along increasing gamma, to the rounding of gamma itself
    assert (np.diff(along) >= -T.BAR * np.abs(along[1:])).all()


def test_clipped_variance_scores_zero(engine):
    """Noise 1e-15 and candidates ON the training points: the true variance there is below the rounding of 1 - |W k*|^2, so the sign
    of the computed one is rounding alone and a good share of the rows clip to sd == 0 (tests/test_gpu_call_order.py uses the same
    model for the negative-variance flag).  A clipped row scores 0; the others hold the bar."""
    rs = np.random.RandomState(3)
    X = rs.uniform(size=(600, 3))[:300]
    yn, ym, ys_ = O.normalize_targets(np.sin(3 * X.sum(axis=1)))
    engine.fit(X, yn, O.MATERN25, 0.7, 1e-15)
    engine.set_candidates(np.vstack([X, rs.uniform(size=(33, 3))]))
    mu, sd = engine.posterior(0, ym, ys_)
    clipped = sd == 0
    print(f"{int(clipped.sum())} of {sd.shape[0]} candidates have a clipped variance")
    assert clipped.any() and not clipped.all()
    engine.take_negative_variance_flag()
    y_star = [float(mu.max()) + 0.01, float(mu.max()) + 0.5]
    bi, bv, si, sv, ys = engine.mes_argbest(y_star, k_seeds=4, return_values=True)
    assert (ys[clipped] == 0).all()
    check_values("clipped", ys, mu, sd, y_star)
    assert not clipped[bi] and not clipped[si].any()          # a point without information is never the pick while another has some


def test_nan_row_wins_and_sorts_last(engine):
    c = case_of("n40-d3-m257")
    Xn = c.Xc.copy()
    Xn[[140, 11], [1, 0]] = np.nan
    mu, sd = c.posterior(engine, Xn)
    assert np.isnan(mu[[11, 140]]).all()
    y_star = c.y_star(np.nan_to_num(mu, nan=Y_MEAN), np.nan_to_num(sd, nan=Y_STD), 5)
    bi, bv, si, sv, ys = engine.mes_argbest(y_star, k_seeds=64, return_values=True)
    assert bi == 11 and np.isnan(bv)
    assert np.isnan(ys[[11, 140]]).all() and np.isfinite(np.delete(ys, [11, 140])).all()
    assert not np.isin([11, 140], si).any()                   # NaNs last: not among the 64 best of 257
    check_values("NaN rows", ys, mu, sd, y_star)
    wi, wv, wsi, wsv = T.argbest(ys, 64)
    assert np.array_equal(si, wsi)


def test_a_candidates_bits_do_not_depend_on_m(engine):
    """The first 257 rows of the M = 1000 set, evaluated as M = 257 (two blocks, one live thread in the second) and inside M = 1000:
    wherever the posterior pass gave a row the same mu / sd bits, its MES value is the same bits."""
    big, small = case_of("n40-d3-m1000"), case_of("n40-d3-m257")
    assert np.array_equal(big.Xc[:257], small.Xc)
    mu_b, sd_b = big.posterior(engine)
    y_star = big.y_star(mu_b, sd_b, 16)
    ys_b = engine.mes_argbest(y_star, return_values=True)[4]
    mu_s, sd_s = small.posterior(engine)
    ys_s = engine.mes_argbest(y_star, return_values=True)[4]
    same = (mu_b[:257] == mu_s) & (sd_b[:257] == sd_s)
    print(f"{int(same.sum())} of 257 rows have the same posterior bits at both M")
    assert same.sum() >= 200, "the posterior's own bits differ between the two M: this test has nothing to compare"
    assert np.array_equal(ys_b[:257][same], ys_s[same])
    # ... and twice the same call: the same bits
    assert np.array_equal(engine.mes_argbest(y_star, return_values=True)[4], ys_s)


# ---- a reader --------------------------------------------------------------------------------------------------------------------
def test_reader_only(engine):
    eng = engine
    c = case_of("n300-d17-m1000")
    mu0, sd0 = c.posterior(eng)
    eng.take_negative_variance_flag()
    y_star = c.y_star(mu0, sd0, 16)
    before = eng.acq_argbest(O.UCB, 2.576, k_seeds=8, return_values=True)
    first = eng.mes_argbest(y_star, k_seeds=8, return_values=True)
    after = eng.acq_argbest(O.UCB, 2.576, k_seeds=8, return_values=True)      # still answers, from the posterior before the call
    assert before[0] == after[0] and before[1] == after[1] and np.array_equal(before[2], after[2])
    assert np.array_equal(before[3], after[3]) and np.array_equal(before[4], after[4])
    again = eng.mes_argbest(y_star, k_seeds=8, return_values=True)            # ... and after another acquisition wrote the values
    assert first[0] == again[0] and first[1] == again[1] and all(np.array_equal(a, b) for a, b in zip(first[2:], again[2:]))
    assert np.array_equal(eng.get_candidate_rows(np.arange(c.M), c.d), c.Xc)
    assert eng.take_negative_variance_flag() is False
    mu1, sd1 = eng.posterior(0, Y_MEAN, Y_STD)
    assert np.array_equal(mu0, mu1) and np.array_equal(sd0, sd1)
    # the refresh after an append still takes its incremental route, to the bits it gives without the call in between
    x_new = np.random.RandomState(5).uniform(size=(2, c.d))
    yn2 = np.concatenate([c.yn, [0.2, -0.4]])

    def arm(with_mes):
        c.posterior(eng)
        if with_mes:
            eng.mes_argbest(y_star, k_seeds=8)
        eng.fit_append(x_new, yn2)
        if with_mes:      # the appended model has no posterior over the candidates yet: refused, and the refusal changes nothing
            with pytest.raises(GpboError, match="run gpbo_posterior for slot 0 first"):
                eng.mes_argbest(y_star)
        return eng.posterior_refresh(0, Y_MEAN, Y_STD, return_route=True)

    mu_a, sd_a, route_a = arm(False)
    mu_b, sd_b, route_b = arm(True)
    assert route_a == 1 and route_b == 1
    assert np.array_equal(mu_a, mu_b) and np.array_equal(sd_a, sd_b)
    ys = eng.mes_argbest(y_star, return_values=True)[4]                        # over the refreshed posterior
    check_values("after the refresh", ys, mu_b, sd_b, y_star)
    assert eng.take_negative_variance_flag() is False


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(engine):
    eng = engine
    c = case_of("n40-d3-m257")
    mu, sd = c.posterior(eng)
    good = c.y_star(mu, sd, 5)
    ref = eng.mes_argbest(good, k_seeds=4, return_values=True)
    for bad in (np.zeros(0), np.zeros(65)):
        with pytest.raises(ValueError, match="n_samples"):
            eng.mes_argbest(bad)
    for bad in (np.nan, np.inf, -np.inf):
        y = good.copy()
        y[3] = bad
        with pytest.raises(ValueError, match="finite"):
            eng.mes_argbest(y)
    for bad in (-1, 65):
        with pytest.raises(ValueError, match="k_seeds"):
            eng.mes_argbest(good, k_seeds=bad)
    with pytest.raises(ValueError):
        eng.mes_argbest(np.zeros((2, 2)))
    # NULL arguments, at the C boundary
    bi, bv = np.empty(1, dtype=np.int64), np.empty(1)
    si, sv = np.empty(4, dtype=np.int64), np.empty(4)
    call = eng._lib.gpbo_mes_argbest
    assert call(eng._h, 5, None, 0, 0, iptr(bi), dptr(bv), None, None, None) == _lib.ERR_INVALID
    assert call(eng._h, 5, dptr(good), 0, 0, None, dptr(bv), None, None, None) == _lib.ERR_INVALID
    assert call(eng._h, 5, dptr(good), 0, 0, iptr(bi), None, None, None, None) == _lib.ERR_INVALID
    assert call(eng._h, 5, dptr(good), 4, 0, iptr(bi), dptr(bv), None, dptr(sv), None) == _lib.ERR_INVALID
    assert call(eng._h, 5, dptr(good), 4, 0, iptr(bi), dptr(bv), iptr(si), None, None) == _lib.ERR_INVALID
    assert call(eng._h, 0, dptr(good), 0, 0, iptr(bi), dptr(bv), None, None, None) == _lib.ERR_INVALID
    assert call(eng._h, 65, dptr(np.zeros(65)), 0, 0, iptr(bi), dptr(bv), None, None, None) == _lib.ERR_INVALID
    assert call(None, 5, dptr(good), 0, 0, iptr(bi), dptr(bv), None, None, None) == _lib.ERR_INVALID
    # k_seeds = 0 with NULL seeds is fine, and no refusal above changed anything
    assert call(eng._h, 5, dptr(good), 0, 0, iptr(bi), dptr(bv), None, None, None) == _lib.GPBO_OK
    assert bi[0] == ref[0] and bv[0] == ref[1]
    now = eng.mes_argbest(good, k_seeds=4, return_values=True)
    assert now[0] == ref[0] and all(np.array_equal(a, b) for a, b in zip(now[2:], ref[2:]))
    # missing state: new candidates without a posterior pass; a refit without one
    eng.set_candidates(c.Xc[:100])
    with pytest.raises(GpboError, match="run gpbo_posterior for slot 0 first"):
        eng.mes_argbest(good)
    assert call(eng._h, 5, dptr(good), 0, 0, iptr(bi), dptr(bv), None, None, None) == _lib.ERR_STATE
    eng.posterior(0, Y_MEAN, Y_STD, fetch=False)
    eng.mes_argbest(good)
    eng.fit(c.X, c.yn, c.kind, c.ls, NOISE)
    with pytest.raises(GpboError, match="run gpbo_posterior for slot 0 first"):
        eng.mes_argbest(good)
    # a posterior of another slot does not serve
    eng.fit(c.X, c.yn, c.kind, c.ls, NOISE, slot=2)
    eng.posterior(2, Y_MEAN, Y_STD, fetch=False)
    with pytest.raises(GpboError, match="slot 0"):
        eng.mes_argbest(good)
    # slot 0 left unfitted by gpbo_lml
    eng.lml(c.X, c.yn, c.kind, c.ls, NOISE)
    with pytest.raises(GpboError, match="slot 0"):
        eng.mes_argbest(good)
    # a context that never had a fit or candidates, then a fit and no candidates
    fresh = GpEngine(0)
    try:
        with pytest.raises(GpboError, match="slot 0"):
            fresh.mes_argbest(good)
        fresh.fit(c.X, c.yn, c.kind, c.ls, NOISE)
        with pytest.raises(GpboError, match="slot 0"):
            fresh.mes_argbest(good)
        assert fresh._lib.gpbo_mes_argbest(fresh._h, 5, dptr(good), 0, 0, iptr(bi), dptr(bv), None, None, None) == _lib.ERR_STATE
    finally:
        fresh.close()
    # a device group
    with pytest.raises(NotImplementedError, match="device group"):
        GroupEngine.mes_argbest(object.__new__(GroupEngine), good)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_suggest_mes_picks_the_truths_maximiser(engine):
    """A driver built the way accelerate() leaves a BayesianOptimization (batch_truth.Driver: HipGPR on slot 0 of the real engine, an
    all-float space, the optimizer's RandomState) on a 2-D target."""
    D, N, M, S = 2, 25, 2000, 8
    bounds = np.array([[0.0, 1.0], [0.0, 1.0]])
    X = bounds[:, 0] + np.random.RandomState(77).uniform(size=(N, D)) * (bounds[:, 1] - bounds[:, 0])
    y = np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1]) - 0.3 * (X[:, 0] - 0.5) ** 2

    def run():
        drv = B.Driver(engine, X, y, bounds, A.UpperConfidenceBound(kappa=2.576), seed=11, n_random=M)
        params, info = suggest_mes(drv, S, n_random=M, n_features=256, refine=4, return_info=True)
        return drv, params, info

    drv, params, info = run()
    gp = drv._gp
    assert drv._acquisition_function.i == 0 and gp.X_train_.shape[0] == N and list(params) == drv._space.keys
    assert info["y_star"].shape == (S,) and np.isfinite(info["y_star"]).all()
    floor = float(y.max()) + 5.0 * np.sqrt(float(gp.alpha)) * float(gp._y_train_std)
    assert (info["y_star"] >= floor).all()
    # the candidates and the fit are still resident: the device's own posterior, and the truth over it
    Xc = engine.get_candidate_rows(np.arange(M), D)
    mu, sd = engine.posterior(0, float(gp._y_train_mean), float(gp._y_train_std))
    assert np.ptp(mu) > 0.5 * np.ptp(y), "the theta search ended at a degenerate model: pick another seed"
    a = T.mes_values(mu, sd, info["y_star"])
    assert T.separated_top(a, 1), "the truth's own best and second best are within the bar: pick another seed"
    assert info["index"] == int(a.argmax())
    assert abs(info["value"] - a.max()) <= T.BAR * a.max() and info["value"] > 0
    assert np.array_equal(np.array(list(params.values())), Xc[info["index"]])
    assert (Xc >= bounds[:, 0]).all() and (Xc <= bounds[:, 1]).all()
    # equal seeds, equal answers
    drv2, params2, info2 = run()
    assert params2 == params and info2["index"] == info["index"] and info2["value"] == info["value"]
    assert np.array_equal(info2["y_star"], info["y_star"])
    sa, sb = drv._random_state.get_state(), drv2._random_state.get_state()
    assert np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]
