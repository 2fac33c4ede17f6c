"""GPU (-m gpu): gpbo_sample_paths — posterior function draws over the resident candidates (Matheron's rule over random Fourier
features) and each draw's maximiser — against tests/paths_truth.py.

Parity.  The error of a (S, M) block of values is  max |f - f_ref| / (y_std max(1, max |f_ref,n|)),  f_ref,n the reference in
normalised-target units.  Tiny cases (N <= 65, M <= 64, F <= 65): the reference is the 50-digit truth and the bar max(1e-9, 8 x
the fp64 restatement's own error against that truth).  Other cases: the reference is the fp64 restatement (cho_solve route) and the
bar max(1e-9, 8 x the spread between the two NumPy routes).  1e-9 is the project's bar; the 8 is the margin for another summation
order.  best_idx is compared only where the truth's own best and second best value are at least 1e-6 of the range apart, asserted
on the truth alone.  The shapes are the edges of the code: the LDS stage of 64 training points / features on both sides, all three
fit tiers (one launch NP <= 64, strips NP <= 768, multi-launch), every padded dimension, every accumulator count (1, 4, 16) with
partly filled ones, the wide workgroup (M >= 2^17), a scaled slot, an F32 slot, a slot after fit_append.  The instance axis — every
(padded width, kernel kind, accumulator count) of path_eval_kernel — is tests/test_gpu_instances.py's.

Exact properties: bitwise repeatability; path s alone = path s among 16; ties to the lowest index; index_offset; the first NaN wins.
Reader only: the resident posterior, the refreshable state, the candidates and the negative-variance flag survive the call."""
import functools

import numpy as np
import pytest

import batch_truth as B
import matern_family_truth as F
import paths_truth as P
from bayesianoptimization_amd import _lib
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd import suggest_thompson
from bayesianoptimization_amd._lib import GpboError
from bayesianoptimization_amd.engine import F32, GpEngine, GroupEngine
from bayesianoptimization_amd.thompson import spectral_draw
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

KNAME = {F.RBF: "rbf", F.MATERN25: "matern25", F.MATERN15: "matern15", F.MATERN05: "matern05"}
NOISE = 1e-4
Y_MEAN, Y_STD = 3.5, 0.4
BAR, MARGIN, GAP_FLOOR = 1e-9, 8.0, 1e-6

#: name -> (N, M, F, d, S, kind, one length scale per dimension, reference)
CASES = {
    "n1-m1-f1-d1-s1": (1, 1, 1, 1, 1, F.RBF, False, "mp"),
    "n63-m63-f63-d2-s2": (63, 63, 63, 2, 2, F.MATERN25, True, "mp"),
    "n64-m63-f64-d5-s5": (64, 63, 64, 5, 5, F.MATERN15, True, "mp"),
    "n65-m1-f65-d1-s16": (65, 1, 65, 1, 16, F.MATERN05, False, "mp"),
    "n130-m257-f1000-d17-s16": (130, 257, 1000, 17, 16, F.RBF, True, "fp64"),
    "n300-m257-f65-d33-s5": (300, 257, 65, 33, 5, F.MATERN25, False, "fp64"),
    "n800-m63-f64-d64-s2": (800, 63, 64, 64, 2, F.MATERN15, True, "fp64"),
    "n65-m131075-f63-d2-s1": (65, (1 << 17) + 3, 63, 2, 1, F.MATERN05, True, "fp64"),
}


def length_scale(d, per_dim):
    s = 0.5 * np.sqrt(d)
    return s * np.geomspace(0.75, 1.33, d) if per_dim else np.array([s])


def err_of(f, ref):
    ref_n = (ref - Y_MEAN) / Y_STD
    return float(np.max(np.abs(f - ref)) / (Y_STD * max(1.0, float(np.max(np.abs(ref_n))))))


class Case:
    """Data, draws and references of one case (computed once, shared, never changed)."""

    def __init__(self, N, M, Fn, d, S, kind, per_dim, reference, amplitude=1.0, white=0.0, seed=0):
        self.N, self.M, self.F, self.d, self.S, self.kind, self.reference = N, M, Fn, d, S, kind, reference
        self.amplitude, self.white = amplitude, white
        self.X, y = F.data(N, d, seed=seed + 17 * N + d)
        self.yn = (y - y.mean()) / y.std() if N > 1 else np.array([0.3])
        self.ls = length_scale(d, per_dim)
        rs = np.random.RandomState(1000 + seed + N + M + Fn)
        self.Xc = rs.uniform(size=(M, d))
        self.omega, self.phase = spectral_draw(kind, Fn, d, rs)
        self.w = rs.standard_normal((S, Fn))
        self.eps = rs.standard_normal((S, N)) * np.sqrt(NOISE + white)
        self.eta = (NOISE + white) / amplitude
        self.what = f"N={N} M={M} F={Fn} d={d} S={S} {KNAME[kind]}"

    def truth_args(self):
        return (self.kind, self.X, self.yn, self.ls, self.eta, self.omega, self.phase, self.w, self.eps, self.Xc, Y_MEAN, Y_STD)

    def references(self):
        """(reference values, bar)"""
        cho = P.paths_cho(*self.truth_args(), amplitude=self.amplitude)
        if self.reference == "mp":
            ref = P.paths_mp(*self.truth_args(), amplitude=self.amplitude)
            own = err_of(cho, ref)
        else:
            ref = cho
            own = err_of(P.paths_winv(*self.truth_args(), amplitude=self.amplitude), cho)
        return ref, max(BAR, MARGIN * own), own

    def fit(self, eng, precision=0):
        scaled = {} if (self.amplitude, self.white) == (1.0, 0.0) else {"amplitude": self.amplitude, "white": self.white}
        eng.fit(self.X, self.yn, self.kind, self.ls, NOISE, precision=precision, **scaled)
        eng.set_candidates(self.Xc)

    def sample(self, eng, **kw):
        return eng.sample_paths(self.omega, self.phase, self.w, self.eps, y_mean=Y_MEAN, y_std=Y_STD, return_values=True, **kw)


@functools.lru_cache(maxsize=None)
def case_of(name):
    c = Case(*CASES[name])
    c.ref, c.bar, c.own = c.references()
    return c


def check(c, idx, val, values, ref, bar, own):
    assert values.shape == (c.S, c.M) and idx.shape == (c.S,) and val.shape == (c.S,)
    e = err_of(values, ref)
    print(f"{c.what}: error {e:.2e}, bar {bar:.2e} (the reference's own {own:.2e})")
    assert e <= bar, f"{c.what}: error {e:.2e} over its bar {bar:.2e}"
    want, gaps = P.argmax_with_gap(ref)
    assert gaps.min() >= GAP_FLOOR, f"{c.what}: the truth's own best / second gap {gaps.min():.2e}: pick another seed"
    assert np.array_equal(idx, want), f"{c.what}: picks {idx.tolist()}, truth {want.tolist()}"
    assert np.array_equal(val, values[np.arange(c.S), idx])          # the value of the pick, the bits of values_out
    return e


@pytest.mark.parametrize("name", list(CASES))
def test_parity(engine, name):
    c = case_of(name)
    c.fit(engine)
    idx, val, values = c.sample(engine)
    check(c, idx, val, values, c.ref, c.bar, c.own)


@functools.lru_cache(maxsize=None)
def scaled_case():
    c = Case(130, 257, 64, 5, 5, F.MATERN25, True, "fp64", amplitude=2.5, white=1e-3)
    c.ref, c.bar, c.own = c.references()
    return c


def test_scaled_slot(engine):
    c = scaled_case()
    c.fit(engine)
    check(c, *c.sample(engine), c.ref, c.bar, c.own)
    # the amplitude is in the prior draw: the unit model's values differ
    unit = P.paths_cho(*c.truth_args(), amplitude=1.0)
    assert err_of(unit, c.ref) > 1e-3


@functools.lru_cache(maxsize=None)
def mid_case():
    c = Case(300, 257, 65, 5, 16, F.MATERN25, False, "fp64")
    c.ref, c.bar, c.own = c.references()
    return c


def test_f32_slot_is_fp64_all_the_same(engine):
    c = mid_case()
    c.fit(engine, precision=F32)
    check(c, *c.sample(engine), c.ref, c.bar, c.own)


def test_after_fit_append(engine):
    N0, rows = 130, 3
    c = Case(N0 + rows, 257, 64, 5, 5, F.MATERN15, True, "fp64")
    ref, bar, own = c.references()
    yn0 = c.yn[:N0] * 1.1 - 0.05          # other targets before the append: every target changes with it
    engine.fit(c.X[:N0], yn0, c.kind, c.ls, NOISE)
    engine.set_candidates(c.Xc)
    engine.fit_append(c.X[N0:], c.yn)
    check(c, *c.sample(engine), ref, bar, own)


# ---- exact properties ----------------------------------------------------------------------------------------------------------
def test_bitwise_repeatable_and_alone_equals_among_sixteen(engine):
    c = mid_case()
    c.fit(engine)
    idx, val, values = c.sample(engine)
    idx2, val2, values2 = c.sample(engine)
    assert np.array_equal(values, values2) and np.array_equal(idx, idx2) and np.array_equal(val, val2)
    for lo, hi in ((0, 1), (7, 8), (15, 16), (4, 8), (2, 5), (3, 16)):        # 1, 4 and 16 accumulators, full and partly filled
        i, v, f = engine.sample_paths(c.omega, c.phase, c.w[lo:hi], c.eps[lo:hi], y_mean=Y_MEAN, y_std=Y_STD, return_values=True)
        assert np.array_equal(f, values[lo:hi]), f"paths {lo}..{hi} alone differ from the same paths among 16"
        assert np.array_equal(i, idx[lo:hi]) and np.array_equal(v, val[lo:hi])
    # values_out not asked for: the same picks
    i, v, f = engine.sample_paths(c.omega, c.phase, c.w, c.eps, y_mean=Y_MEAN, y_std=Y_STD)
    assert f is None and np.array_equal(i, idx) and np.array_equal(v, val)


def test_zero_draws_give_the_posterior_mean(engine):
    c = mid_case()
    c.fit(engine)
    mu, _ = engine.posterior(0, Y_MEAN, Y_STD)
    _, _, values = engine.sample_paths(c.omega, c.phase, np.zeros((2, c.F)), np.zeros((2, c.N)), y_mean=Y_MEAN, y_std=Y_STD,
                                       return_values=True)
    want = P.posterior_mean(c.kind, c.X, c.yn, c.ls, c.eta, c.Xc, Y_MEAN, Y_STD)
    print(f"{c.what}: zero draws vs gpbo_posterior {err_of(values[0], mu):.2e}, vs the truth {err_of(values[0], want):.2e}")
    assert np.array_equal(values[0], values[1])
    assert err_of(values[0], mu) <= c.bar and err_of(values[0], want) <= c.bar


def test_ties_offset_and_nan(engine):
    c = case_of("n63-m63-f63-d2-s2")
    c.fit(engine)
    idx, val, values = c.sample(engine)
    # every candidate twice: the copy's values are the original's bits, the pick is the lower index
    engine.set_candidates(np.vstack([c.Xc, c.Xc]))
    idx2, val2, values2 = c.sample(engine)
    assert np.array_equal(values2[:, :c.M], values) and np.array_equal(values2[:, c.M:], values)
    assert np.array_equal(idx2, idx) and np.array_equal(val2, val)
    # index_offset is added
    idx3, val3, _ = c.sample(engine, index_offset=10**10)
    assert np.array_equal(idx3, idx + 10**10) and np.array_equal(val3, val)
    # a candidate with a NaN coordinate is the pick of every path (the first of two)
    Xn = c.Xc.copy()
    Xn[[40, 11], [1, 0]] = np.nan
    engine.set_candidates(Xn)
    idx4, val4, values4 = c.sample(engine)
    assert np.array_equal(idx4, np.full(c.S, 11)) and np.isnan(val4).all()
    assert np.isnan(values4[:, [11, 40]]).all() and np.isfinite(np.delete(values4, [11, 40], axis=1)).all()


# ---- a reader --------------------------------------------------------------------------------------------------------------------
def test_reader_only(engine):
    eng = engine
    c = mid_case()
    c.fit(eng)
    eng.posterior(0, Y_MEAN, Y_STD, fetch=False)
    eng.take_negative_variance_flag()
    before = eng.acq_argbest(O.UCB, 2.576, k_seeds=8, return_values=True)
    c.sample(eng)
    after = eng.acq_argbest(O.UCB, 2.576, k_seeds=8, return_values=True)      # still answers, from the posterior before the call
    assert before[0] == after[0] and before[1] == after[1] and np.array_equal(before[2], after[2])
    assert np.array_equal(before[3], after[3]) and np.array_equal(before[4], after[4])
    assert np.array_equal(eng.get_candidate_rows(np.arange(c.M), c.d), c.Xc)
    assert eng.take_negative_variance_flag() is False
    # an append, the paths of the grown model, and the refresh still takes its incremental route, to the bits it gives without the call
    x_new = np.random.RandomState(5).uniform(size=(2, c.d))
    yn2 = np.concatenate([c.yn, [0.2, -0.4]])
    eps2 = np.hstack([c.eps, np.zeros((c.S, 2))])

    def arm():
        c.fit(eng)
        eng.posterior(0, Y_MEAN, Y_STD, fetch=False)
        eng.fit_append(x_new, yn2)

    arm()
    mu_a, sd_a, route_a = eng.posterior_refresh(0, Y_MEAN, Y_STD, return_route=True)
    arm()
    eng.sample_paths(c.omega, c.phase, c.w, eps2, y_mean=Y_MEAN, y_std=Y_STD)
    mu_b, sd_b, route_b = eng.posterior_refresh(0, Y_MEAN, Y_STD, return_route=True)
    assert route_a == 1 and route_b == 1
    assert np.array_equal(mu_a, mu_b) and np.array_equal(sd_a, sd_b)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(engine):
    eng = engine
    c = case_of("n63-m63-f63-d2-s2")
    c.fit(eng)
    kw = {"y_mean": Y_MEAN, "y_std": Y_STD}
    for n_paths in (0, 17):
        with pytest.raises(ValueError, match="n_paths"):
            eng.sample_paths(c.omega, c.phase, np.zeros((n_paths, c.F)), np.zeros((n_paths, c.N)), **kw)
    with pytest.raises(ValueError, match="n_features"):
        eng.sample_paths(np.zeros((0, c.d)), np.zeros(0), np.zeros((1, 0)), np.zeros((1, c.N)), **kw)
    with pytest.raises(ValueError, match="n_features"):
        eng.sample_paths(np.zeros((4097, c.d)), np.zeros(4097), np.zeros((1, 4097)), np.zeros((1, c.N)), **kw)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="y_std"):
            eng.sample_paths(c.omega, c.phase, c.w, c.eps, y_std=bad)
    with pytest.raises(ValueError):       # shapes that do not fit the slot's model never reach the library
        eng.sample_paths(c.omega, c.phase, c.w, c.eps[:, :-1], **kw)
    with pytest.raises(ValueError):
        eng.sample_paths(c.omega[:, :1], c.phase, c.w, c.eps, **kw)
    # a NULL input, at the C boundary
    from bayesianoptimization_amd._lib import dptr, iptr

    bi, bv = np.empty(c.S, dtype=np.int64), np.empty(c.S)
    ptrs = [dptr(c.omega), dptr(c.phase), dptr(np.ascontiguousarray(c.w)), dptr(np.ascontiguousarray(c.eps))]
    for k in range(4):
        a = list(ptrs)
        a[k] = None
        rc = eng._lib.gpbo_sample_paths(eng._h, 0, Y_MEAN, Y_STD, c.S, c.F, *a, 0, iptr(bi), dptr(bv), None)
        assert rc == _lib.ERR_INVALID
    assert eng._lib.gpbo_sample_paths(eng._h, 0, Y_MEAN, Y_STD, c.S, c.F, *ptrs, 0, None, dptr(bv), None) == _lib.ERR_INVALID
    assert eng._lib.gpbo_sample_paths(eng._h, 0, Y_MEAN, Y_STD, c.S, c.F, *ptrs, 0, iptr(bi), None, None) == _lib.ERR_INVALID
    # a slot that gpbo_lml left unfitted
    eng.fit(c.X, c.yn, c.kind, c.ls, NOISE, slot=3)
    eng.lml(c.X, c.yn, c.kind, c.ls, NOISE, slot=3)
    with pytest.raises(GpboError, match="not been fitted"):
        eng.sample_paths(c.omega, c.phase, c.w, c.eps, slot=3, **kw)
    assert eng._lib.gpbo_sample_paths(eng._h, 3, Y_MEAN, Y_STD, c.S, c.F, *ptrs, 0, iptr(bi), dptr(bv), None) == _lib.ERR_STATE
    # a fit pending on the slot (the engine would wait for it: asked at the C boundary)
    with eng.overlapped_fits():
        eng.fit(c.X, c.yn, c.kind, c.ls, NOISE)
        rc = eng._lib.gpbo_sample_paths(eng._h, 0, Y_MEAN, Y_STD, c.S, c.F, *ptrs, 0, iptr(bi), dptr(bv), None)
        assert rc == _lib.ERR_STATE
    # candidates of another d
    eng.set_candidates(np.random.RandomState(1).uniform(size=(10, c.d + 1)))
    with pytest.raises(GpboError, match="dimension"):
        eng.sample_paths(c.omega, c.phase, c.w, c.eps, **kw)
    # no resident candidates: a context that never had any
    fresh = GpEngine(0)
    try:
        with pytest.raises(GpboError, match="not been fitted"):      # ... and a slot that never was fitted
            fresh.sample_paths(c.omega, c.phase, c.w, c.eps, slot=5, **kw)
        assert fresh._lib.gpbo_sample_paths(fresh._h, 5, Y_MEAN, Y_STD, c.S, c.F, *ptrs, 0, iptr(bi), dptr(bv), None) == _lib.ERR_STATE
        fresh.fit(c.X, c.yn, c.kind, c.ls, NOISE)
        with pytest.raises(GpboError, match="no candidates"):
            fresh.sample_paths(c.omega, c.phase, c.w, c.eps, **kw)
    finally:
        fresh.close()
    # a device group
    with pytest.raises(NotImplementedError, match="device group"):
        GroupEngine.sample_paths(object.__new__(GroupEngine), c.omega, c.phase, c.w, c.eps)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_suggest_thompson_picks_the_truths_maximisers(engine):
    D, N, M, Q, FEATURES = 3, 30, 2000, 5, 256
    bounds = np.array([[0.0, 1.0]] * D)
    X = np.random.RandomState(130).uniform(size=(N, D))
    y = np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1]) + X[:, 2] ** 2

    def driver():
        return B.Driver(engine, X, y, bounds, A.UpperConfidenceBound(kappa=2.576), seed=7, n_random=M)

    drv = driver()
    picks = suggest_thompson(drv, Q, n_random=M, n_features=FEATURES)
    Xc = engine.get_candidate_rows(np.arange(M), D)                           # the one candidate draw is still resident
    gp = drv._gp
    assert drv._acquisition_function.i == 0 and gp.X_train_.shape[0] == N
    # the documented draws, replayed on a twin RandomState: the theta search, the candidates, the features, weights and noise
    twin = driver()
    twin._gp.fit(twin._space.params, twin._space.target)
    rng = twin._random_state
    assert np.array_equal(np.column_stack([rng.uniform(0.0, 1.0, M) for _ in range(D)]), Xc)
    assert int(twin._gp._kind) == int(gp._kind) and np.array_equal(twin._gp._ls, gp._ls)
    omega, phase = spectral_draw(gp._kind, FEATURES, D, rng)
    w = rng.standard_normal((Q, FEATURES))
    eps = rng.standard_normal((Q, N)) * np.sqrt(float(gp.alpha))
    yn = (y - gp._y_train_mean) / gp._y_train_std
    vals = P.paths_cho(int(gp._kind), X, yn, np.array(gp._ls), float(gp.alpha), omega, phase, w, eps, Xc, gp._y_train_mean,
                       gp._y_train_std)
    want, gaps = P.argmax_with_gap(vals)
    got = B.rows_to_indices(picks, Xc)
    print(f"picks {got.tolist()} truth {want.tolist()} gaps {['%.1e' % g for g in gaps]}")
    assert gaps.min() >= GAP_FLOOR, f"the truth's own best / second gap {gaps.min():.2e}: pick another seed"
    assert np.array_equal(got, want)
    a, b = drv._random_state.get_state(), rng.get_state()
    assert np.array_equal(a[1], b[1]) and a[2:] == b[2:]
