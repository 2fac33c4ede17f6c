"""GPU (-m gpu): gpbo_sample_paths_constrained — the draws of the objective and of C constraints over the resident candidates, the
violation folded on the device and the constrained pick per draw — against gpbo_sample_paths and tests/scbo_truth.py.

Same bits: values_out[j] is what sample_paths(slot=j) returns for the same inputs, at the edges of the code (both sides of the LDS
stage of 64, differing N per slot, three kernel kinds, C = 7, the wide workgroup, a scaled and an F32 slot among the constraints).
Violation: viol_out against the NumPy rule on the device's OWN values_out — the zero pattern exactly, the other entries within
4 ulp of the largest term (the rule is a maximum, one division and C - 1 additions per entry; with C = 1 nothing rounds twice).
Picks: exactly the rule's on the device's own values_out / viol_out, for bounds taken from the truth's values (tests/paths_truth.py).
Exact properties, reader only, refusals, and suggest_constrained_thompson end to end against the truth."""
import functools
import warnings

import numpy as np
import pytest

import batch_truth as B
import matern_family_truth as F
import paths_truth as P
import scbo_truth as ST
from bayesianoptimization_amd import _lib
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd import suggest_constrained_thompson
from bayesianoptimization_amd._lib import GpboError, dptr, iptr
from bayesianoptimization_amd.constraint_model import HipConstraintModel
from bayesianoptimization_amd.engine import F32, GpEngine, GroupEngine
from bayesianoptimization_amd.float_space import FloatSpace
from bayesianoptimization_amd.thompson import spectral_draw
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

NOISE = 1e-4
INF = np.inf
GAP_FLOOR = 1e-6
KINDS = (F.MATERN25, F.RBF, F.MATERN15, F.MATERN05)


@pytest.fixture(scope="module")
def engine():
    """A context of this module's own: its cases fit every slot up to 7, and the suite's shared context has tests that count on
    slots nobody has fitted."""
    eng = GpEngine(0)
    yield eng
    eng.close()


def length_scale(d, per_dim, j):
    s = 0.5 * np.sqrt(d) * (1.0 + 0.15 * j)
    return s * np.geomspace(0.75, 1.33, d) if per_dim else np.array([s])


class Setup:
    """1 + C slots' data, fits' arguments and draws over one candidate set (computed once, shared, never changed).  Slot j: N[j]
    observations, kind kinds[j], its own length scales, y_mean = 3.5 - j, y_std = 0.4 + 0.3 j."""

    def __init__(self, C, Ns, M, Fn, S, d, kinds=None, per_dim=False, scaled_slot=None, f32_slot=None, seed=0):
        self.C, self.M, self.F, self.S, self.d = C, M, Fn, S, d
        self.Ns = [Ns] * (1 + C) if np.isscalar(Ns) else list(Ns)
        self.kinds = [KINDS[0]] * (1 + C) if kinds is None else list(kinds)
        self.scaled_slot, self.f32_slot = scaled_slot, f32_slot
        rs = np.random.RandomState(4000 + seed + 7 * C + M + Fn)
        self.Xc = rs.uniform(size=(M, d))
        self.y_mean = np.array([3.5 - j for j in range(1 + C)])
        self.y_std = np.array([0.4 + 0.3 * j for j in range(1 + C)])
        self.slots, self.draws = [], []
        for j in range(1 + C):
            N = self.Ns[j]
            X, y = F.data(N, d, seed=seed + 17 * N + d + 101 * j)
            yn = (y - y.mean()) / y.std()
            amplitude, white = (2.5, 1e-3) if j == scaled_slot else (1.0, 0.0)
            self.slots.append(dict(X=X, yn=yn, kind=self.kinds[j], ls=length_scale(d, per_dim, j), amplitude=amplitude, white=white,
                                   precision=F32 if j == f32_slot else 0))
            omega, phase = spectral_draw(self.kinds[j], Fn, d, rs)
            self.draws.append((omega, phase, rs.standard_normal((S, Fn)), rs.standard_normal((S, N)) * np.sqrt(NOISE + white)))
        self.what = f"C={C} N={self.Ns} M={M} F={Fn} S={S} d={d}"

    def fit(self, eng, Xc=None):
        for j, s in enumerate(self.slots):
            scaled = {} if (s["amplitude"], s["white"]) == (1.0, 0.0) else {"amplitude": s["amplitude"], "white": s["white"]}
            eng.fit(s["X"], s["yn"], s["kind"], s["ls"], NOISE, slot=j, precision=s["precision"], **scaled)
        eng.set_candidates(self.Xc if Xc is None else Xc)

    def run(self, eng, lb, ub, rows=None, **kw):
        draws = self.draws if rows is None else [(o, p, w[rows], e[rows]) for o, p, w, e in self.draws]
        kw.setdefault("return_values", True)
        return eng.sample_paths_constrained(draws, np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64), self.y_mean,
                                            self.y_std, **kw)

    def plain(self, eng, j):
        o, p, w, e = self.draws[j]
        return eng.sample_paths(o, p, w, e, slot=j, y_mean=self.y_mean[j], y_std=self.y_std[j], return_values=True)

    @functools.lru_cache(maxsize=None)
    def truth(self):
        """(1 + C, S, M) by paths_cho"""
        out = []
        for j, (s, (o, p, w, e)) in enumerate(zip(self.slots, self.draws)):
            eta = (NOISE + s["white"]) / s["amplitude"]
            out.append(P.paths_cho(s["kind"], s["X"], s["yn"], s["ls"], eta, o, p, w, e, self.Xc, self.y_mean[j], self.y_std[j],
                                   amplitude=s["amplitude"]))
        return np.array(out)


#: name -> Setup arguments: the smallest shapes that reach each edge of the code
CASES = {
    "c1-n63,65-m63-f63-s1-d2": dict(C=1, Ns=(63, 65), M=63, Fn=63, S=1, d=2),
    "c2-n130-m257-f65-s5-d5": dict(C=2, Ns=130, M=257, Fn=65, S=5, d=5, kinds=(F.MATERN25, F.RBF, F.MATERN15), per_dim=True),
    "c7-n130-m63-f64-s16-d17": dict(C=7, Ns=130, M=63, Fn=64, S=16, d=17),
    "c1-n65-m131075-f63-s4-d2": dict(C=1, Ns=65, M=(1 << 17) + 3, Fn=63, S=4, d=2, kinds=(F.MATERN05, F.MATERN25)),
    "c2-n130-m257-f64-s5-d5-scaled-f32": dict(C=2, Ns=(130, 100, 70), M=257, Fn=64, S=5, d=5, per_dim=True, scaled_slot=1, f32_slot=2),
    "c1-n63,65-m257-f64-s5-d2": dict(C=1, Ns=(63, 65), M=257, Fn=64, S=5, d=2),
    "c2-n130-m257-f64-s16-d5": dict(C=2, Ns=(130, 65, 130), M=257, Fn=64, S=16, d=5),
}


@functools.lru_cache(maxsize=None)
def setup_of(name):
    return Setup(**CASES[name])


def check_rule(c, out, lb, ub, index_offset=0):
    """viol_out against the rule on the device's own values_out, the picks exactly the rule's on values_out / viol_out"""
    idx, val, bv, feas, values, viol = out
    S = values.shape[1]
    assert values.shape == (1 + c.C, S, values.shape[2]) and viol.shape == values.shape[1:]
    assert idx.shape == val.shape == bv.shape == feas.shape == (S,) and feas.dtype == bool
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    want = ST.violations(values, lb, ub, c.y_std)
    with np.errstate(invalid="ignore"):
        terms = np.array([np.maximum(np.maximum(lb[j] - values[j + 1], values[j + 1] - ub[j]), 0.0) / c.y_std[j + 1] for j in range(c.C)])
    assert np.array_equal(viol == 0.0, want == 0.0) and np.array_equal(np.isnan(viol), np.isnan(want))
    ok = ~np.isnan(want)
    ulps = np.abs(viol - want)[ok] / np.spacing(np.max(terms, axis=0))[ok]
    print(f"{c.what}: violation off by at most {ulps.max() if ulps.size else 0.0:.2f} ulp of the largest term; "
          f"feasible per path {(want == 0.0).mean(axis=1).round(3).tolist()}")
    assert (ulps <= 4.0).all()
    i2, v2, b2, f2 = ST.picks(values[0], viol, index_offset)
    assert np.array_equal(idx, i2) and np.array_equal(feas, f2), f"{c.what}: picks {idx.tolist()}, the rule's {i2.tolist()}"
    assert np.array_equal(val, v2, equal_nan=True) and np.array_equal(bv, b2, equal_nan=True)
    return want


# ---- the same bits as gpbo_sample_paths -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES)[:5])
def test_values_are_sample_paths_bits(engine, name):
    c = setup_of(name)
    c.fit(engine)
    out = c.run(engine, np.full(c.C, -0.5) + c.y_mean[1:], np.full(c.C, 0.5) + c.y_mean[1:])
    check_rule(c, out, np.full(c.C, -0.5) + c.y_mean[1:], np.full(c.C, 0.5) + c.y_mean[1:])
    for j in range(1 + c.C):
        _, _, f = c.plain(engine, j)
        assert np.array_equal(out[4][j], f), f"{c.what}: slot {j}'s values differ from sample_paths'"
    # nothing asked for: the same picks
    idx, val, bv, feas, values, viol = c.run(engine, np.full(c.C, -0.5) + c.y_mean[1:], np.full(c.C, 0.5) + c.y_mean[1:], return_values=False)
    assert values is None and viol is None
    assert np.array_equal(idx, out[0]) and np.array_equal(val, out[1]) and np.array_equal(bv, out[2]) and np.array_equal(feas, out[3])


# ---- the picks ---------------------------------------------------------------------------------------------------------------------
def quantile_bounds(c, lo, hi):
    t = c.truth()
    return (np.array([np.quantile(t[j], lo) for j in range(1, 1 + c.C)]), np.array([np.quantile(t[j], hi) for j in range(1, 1 + c.C)]))


def test_picks_a_few_per_cent_feasible(engine):
    c = setup_of("c2-n130-m257-f65-s5-d5")
    lb, ub = quantile_bounds(c, 0.4, 0.6)
    share = (ST.violations(c.truth(), lb, ub, c.y_std) == 0.0).mean(axis=1)
    assert (share > 0.01).all() and (share < 0.15).all(), f"the truth's feasible share per path {share.tolist()}: pick another seed"
    c.fit(engine)
    out = c.run(engine, lb, ub)
    check_rule(c, out, lb, ub)
    assert out[3].all() and (out[2] == 0.0).all()
    # a feasible pick is not the unconstrained maximiser everywhere: the constraint is what decided
    assert not np.array_equal(out[0], c.plain(engine, 0)[0])


def test_picks_one_path_without_a_feasible_candidate(engine):
    c = setup_of("c1-n63,65-m257-f64-s5-d2")
    minima = np.sort(c.truth()[1].min(axis=1))
    span = np.ptp(c.truth()[1])
    assert (minima[-1] - minima[-2]) / span >= GAP_FLOOR, "the truth's two largest path minima are too close: pick another seed"
    ub = np.array([0.5 * (minima[-1] + minima[-2])])
    c.fit(engine)
    out = c.run(engine, [-INF], ub)
    check_rule(c, out, [-INF], ub)
    dry = int(np.argmax(c.truth()[1].min(axis=1)))
    assert out[3].tolist() == [s != dry for s in range(c.S)] and out[2][dry] > 0.0
    assert out[0][dry] == int(np.argmin(out[4][1][dry]))             # one upper bound: the least violation is the least value


def test_picks_nothing_feasible_and_one_sided_bounds(engine):
    c = setup_of("c2-n130-m257-f65-s5-d5")
    t = c.truth()
    c.fit(engine)
    top = np.array([t[1].max(), t[2].max()]) + 1.0
    out = c.run(engine, top, [INF, INF])                               # nothing feasible
    check_rule(c, out, top, [INF, INF])
    assert not out[3].any() and (out[2] > 0.0).all()
    med = np.array([np.median(t[1]), np.median(t[2])])
    for lb, ub in (([-INF, -INF], med), (med, [INF, INF]), ([-INF, med[1]], [med[0], INF])):
        out = c.run(engine, lb, ub)
        want = check_rule(c, out, lb, ub)
        assert (want == 0.0).any() and not (want == 0.0).all()


def test_picks_infinite_bounds_are_sample_paths_picks(engine):
    c = setup_of("c2-n130-m257-f65-s5-d5")
    c.fit(engine)
    out = c.run(engine, [-INF, -INF], [INF, INF])
    check_rule(c, out, [-INF, -INF], [INF, INF])
    idx, val, _ = c.plain(engine, 0)
    assert np.array_equal(out[0], idx) and np.array_equal(out[1], val) and out[3].all() and (out[5] == 0.0).all()


# ---- exact properties ------------------------------------------------------------------------------------------------------------
def test_bitwise_repeatable_and_alone_equals_among_sixteen(engine):
    c = setup_of("c2-n130-m257-f64-s16-d5")
    lb, ub = quantile_bounds(c, 0.3, 0.7)
    c.fit(engine)
    a = c.run(engine, lb, ub)
    b = c.run(engine, lb, ub)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    check_rule(c, a, lb, ub)
    for lo, hi in ((0, 1), (15, 16), (4, 8), (2, 5), (3, 16)):        # 1, 4 and 16 accumulators, full and partly filled
        o = c.run(engine, lb, ub, rows=slice(lo, hi))
        assert np.array_equal(o[4], a[4][:, lo:hi]) and np.array_equal(o[5], a[5][lo:hi]), f"paths {lo}..{hi} alone differ"
        assert all(np.array_equal(x, y[lo:hi]) for x, y in zip(o[:4], a[:4]))


def test_ties_offset_and_nan(engine):
    c = setup_of("c1-n63,65-m257-f64-s5-d2")
    t = c.truth()
    c.fit(engine)
    for lb, ub in (([-INF], [np.median(t[1])]), ([t[1].max() + 1.0], [INF])):       # the feasible and the infeasible branch
        a = c.run(engine, lb, ub)
        assert a[3].all() or not a[3].any()
        c.fit(engine, np.vstack([c.Xc, c.Xc]))                       # every candidate twice: the pick is the lower index
        b = c.run(engine, lb, ub)
        assert np.array_equal(b[4][:, :, :c.M], a[4]) and np.array_equal(b[4][:, :, c.M:], a[4])
        assert np.array_equal(b[5][:, :c.M], a[5]) and np.array_equal(b[5][:, c.M:], a[5])
        assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4]))
        c.fit(engine)
        o = c.run(engine, lb, ub, index_offset=10**10)                # index_offset is added
        assert np.array_equal(o[0], a[0] + 10**10) and all(np.array_equal(x, y) for x, y in zip(o[1:4], a[1:4]))
        check_rule(c, o, lb, ub, index_offset=10**10)
        Xn = c.Xc.copy()                                              # a NaN coordinate wins, the first of two
        Xn[[40, 11], [1, 0]] = np.nan
        c.fit(engine, Xn)
        n = c.run(engine, lb, ub)
        assert np.array_equal(n[0], np.full(c.S, 11)) and np.isnan(n[1]).all() and np.isnan(n[2]).all() and not n[3].any()
        assert np.isnan(n[5][:, [11, 40]]).all() and np.isfinite(np.delete(n[5], [11, 40], axis=1)).all()
        c.fit(engine)


# ---- a reader --------------------------------------------------------------------------------------------------------------------
def test_reader_only(engine):
    eng = engine
    c = setup_of("c2-n130-m257-f65-s5-d5")
    lb, ub = quantile_bounds(c, 0.3, 0.7)
    c.fit(eng)
    post = [eng.posterior(j, c.y_mean[j], c.y_std[j]) for j in range(1 + c.C)]
    eng.take_negative_variance_flag()
    before = eng.acq_argbest(O.UCB, 2.576, lb=lb, ub=ub, k_seeds=8, return_values=True)
    c.run(eng, lb, ub)
    after = eng.acq_argbest(O.UCB, 2.576, lb=lb, ub=ub, k_seeds=8, return_values=True)    # from the posteriors before the call
    assert before[0] == after[0] and before[1] == after[1] and np.array_equal(before[2], after[2])
    assert np.array_equal(before[3], after[3]) and np.array_equal(before[4], after[4])
    assert np.array_equal(eng.get_candidate_rows(np.arange(c.M), c.d), c.Xc)
    assert eng.take_negative_variance_flag() is False
    for j in range(1 + c.C):                                          # every slot still answers with the bits it gave before
        mu, sd = eng.posterior(j, c.y_mean[j], c.y_std[j])
        assert np.array_equal(mu, post[j][0]) and np.array_equal(sd, post[j][1])
    # an append to slot 0, the call on the grown model, and the refresh still takes its incremental route, to the bits without the call
    s0 = c.slots[0]
    x_new = np.random.RandomState(5).uniform(size=(2, c.d))
    yn2 = np.concatenate([s0["yn"], [0.2, -0.4]])
    o, p, w, e = c.draws[0]
    draws2 = [(o, p, w, np.hstack([e, np.zeros((c.S, 2))]))] + c.draws[1:]

    def arm():
        c.fit(eng)
        eng.posterior(0, c.y_mean[0], c.y_std[0], fetch=False)
        eng.fit_append(x_new, yn2)

    arm()
    mu_a, sd_a, route_a = eng.posterior_refresh(0, c.y_mean[0], c.y_std[0], return_route=True)
    arm()
    eng.sample_paths_constrained(draws2, lb, ub, c.y_mean, c.y_std)
    mu_b, sd_b, route_b = eng.posterior_refresh(0, c.y_mean[0], c.y_std[0], return_route=True)
    assert route_a == 1 and route_b == 1
    assert np.array_equal(mu_a, mu_b) and np.array_equal(sd_a, sd_b)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(engine):
    eng = engine
    c = setup_of("c1-n63,65-m257-f64-s5-d2")
    c.fit(eng)
    lb, ub = np.array([-1.0]), np.array([1.0])
    N0, N1 = c.Ns

    def zeros(S, Fn):
        return [(np.zeros((Fn, c.d)), np.zeros(Fn), np.zeros((S, Fn)), np.zeros((S, N))) for N in (N0, N1)]

    for C in (0, 8):
        with pytest.raises(ValueError, match="draws must be|n_constraints"):
            eng.sample_paths_constrained(c.draws[:1] * (1 + C), np.zeros(C), np.ones(C), np.zeros(1 + C), np.ones(1 + C))
    for n_paths in (0, 17):
        with pytest.raises(ValueError, match="n_paths"):
            eng.sample_paths_constrained(zeros(n_paths, c.F), lb, ub, c.y_mean, c.y_std)
    for n_features in (0, 4097):
        with pytest.raises(ValueError, match="n_features"):
            eng.sample_paths_constrained(zeros(1, n_features), lb, ub, c.y_mean, c.y_std)
    for slot in (0, 1):
        for bad in (0.0, -1.0, np.inf, np.nan):
            y_std = c.y_std.copy()
            y_std[slot] = bad
            with pytest.raises(ValueError, match="y_std"):
                eng.sample_paths_constrained(c.draws, lb, ub, c.y_mean, y_std)
        for bad in (np.inf, np.nan):
            y_mean = c.y_mean.copy()
            y_mean[slot] = bad
            with pytest.raises(ValueError, match="y_mean"):
                eng.sample_paths_constrained(c.draws, lb, ub, y_mean, c.y_std)
    for bad_lb, bad_ub in (([np.nan], [1.0]), ([0.0], [np.nan]), ([1.0], [1.0]), ([2.0], [1.0]), ([INF], [INF]), ([-INF], [-INF])):
        with pytest.raises(ValueError, match="bounds"):
            eng.sample_paths_constrained(c.draws, bad_lb, bad_ub, c.y_mean, c.y_std)
    o, p, w, e = c.draws[1]
    with pytest.raises(ValueError):       # shapes that do not fit a slot's model never reach the library
        eng.sample_paths_constrained([c.draws[0], (o, p, w, e[:, :-1])], lb, ub, c.y_mean, c.y_std)
    with pytest.raises(ValueError):
        eng.sample_paths_constrained([c.draws[0], (o[:, :1], p, w, e)], lb, ub, c.y_mean, c.y_std)
    with pytest.raises(ValueError):
        eng.sample_paths_constrained([c.draws[0], (o, p, w[:2], e[:2])], lb, ub, c.y_mean, c.y_std)
    # NULL arguments, at the C boundary
    S, Fn = c.S, c.F
    cat = [np.ascontiguousarray(np.concatenate([np.ravel(t[k]) for t in c.draws])) for k in range(4)]
    bi, bv, bo = np.empty(S, dtype=np.int64), np.empty(S), np.empty(S)
    fe = np.zeros(S, dtype=np.int32)
    import ctypes

    args = [dptr(c.y_mean), dptr(c.y_std), dptr(lb), dptr(ub), S, Fn, dptr(cat[0]), dptr(cat[1]), dptr(cat[2]), dptr(cat[3]), 0,
            iptr(bi), dptr(bv), dptr(bo), fe.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), None, None]
    call = eng._lib.gpbo_sample_paths_constrained
    assert call(eng._h, 1, *args) == _lib.GPBO_OK
    for k in (0, 1, 2, 3, 6, 7, 8, 9, 11, 12, 13, 14):
        a = list(args)
        a[k] = None
        assert call(eng._h, 1, *a) == _lib.ERR_INVALID, k
    assert call(eng._h, 0, *args) == _lib.ERR_INVALID and call(eng._h, 8, *args) == _lib.ERR_INVALID
    assert call(None, 1, *args) == _lib.ERR_INVALID
    # a fit pending on a slot (the engine would wait for it: asked at the C boundary)
    s1 = c.slots[1]
    with eng.overlapped_fits():
        eng.fit(s1["X"], s1["yn"], s1["kind"], s1["ls"], NOISE, slot=1)
        assert call(eng._h, 1, *args) == _lib.ERR_STATE
    # a slot that gpbo_lml left unfitted
    eng.lml(s1["X"], s1["yn"], s1["kind"], s1["ls"], NOISE, slot=1)
    with pytest.raises(GpboError, match="not been fitted"):
        c.run(eng, lb, ub)
    assert call(eng._h, 1, *args) == _lib.ERR_STATE
    # a slot of another d than the candidates' (the same N: asked at the C boundary, the engine refuses the shapes first)
    eng.fit(np.hstack([s1["X"], s1["X"][:, :1]]), s1["yn"], s1["kind"], s1["ls"][:1], NOISE, slot=1)
    assert call(eng._h, 1, *args) == _lib.ERR_STATE
    with pytest.raises(ValueError):
        c.run(eng, lb, ub)
    # candidates of another d
    c.fit(eng, np.random.RandomState(1).uniform(size=(10, c.d + 1)))
    with pytest.raises(GpboError, match="dimension"):
        c.run(eng, lb, ub)
    # no resident candidates: a context that never had any
    fresh = GpEngine(0)
    try:
        with pytest.raises(GpboError, match="not been fitted"):
            c.run(fresh, lb, ub)
        assert call(fresh._h, 1, *args) == _lib.ERR_STATE
        for j, s in enumerate(c.slots):
            fresh.fit(s["X"], s["yn"], s["kind"], s["ls"], NOISE, slot=j)
        with pytest.raises(GpboError, match="no candidates"):
            c.run(fresh, lb, ub)
    finally:
        fresh.close()
    # a device group
    with pytest.raises(NotImplementedError, match="device group"):
        GroupEngine.sample_paths_constrained(object.__new__(GroupEngine), c.draws, lb, ub, c.y_mean, c.y_std)
    c.fit(eng)
    check_rule(c, c.run(eng, lb + c.y_mean[1], ub + c.y_mean[1]), lb + c.y_mean[1], ub + c.y_mean[1])      # and it still works


# ---- end to end -------------------------------------------------------------------------------------------------------------------
E2E = dict(D=3, N=30, M=2000, Q=5, FEATURES=256, SEED=8, LB=0.0, UB=INF)


def e2e_driver(engine):
    D, N = E2E["D"], E2E["N"]
    bounds = np.array([[0.0, 1.0]] * D)
    X = np.random.RandomState(130).uniform(size=(N, D))
    y = np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1]) + X[:, 2] ** 2
    cv = np.cos(2.0 * X.sum(1))
    drv = B.Driver(engine, X, y, bounds, A.UpperConfidenceBound(kappa=2.576), seed=E2E["SEED"], n_random=E2E["M"])
    cm = HipConstraintModel(None, np.array([E2E["LB"]]), np.array([E2E["UB"]]), engine=engine, random_state=np.random.RandomState(3))
    drv._space = FloatSpace({f"x{j}": tuple(b) for j, b in enumerate(bounds)}, constraint=cm)
    drv._space.register_bulk(X, y, cv)
    return drv, X, y, cv


def e2e_truth(twin, X, y, cv, Xc):
    """(the rule's picks on paths_cho, the truth's own gaps) after the documented draws on the twin's RandomState"""
    Q, FEATURES, N, D = E2E["Q"], E2E["FEATURES"], E2E["N"], E2E["D"]
    rng = twin._random_state
    gps = [twin._gp, twin._space.constraint.model[0]]
    vals = []
    for g, t in zip(gps, (y, cv)):
        omega, phase = spectral_draw(g._kind, FEATURES, D, rng)
        w = rng.standard_normal((Q, FEATURES))
        eps = rng.standard_normal((Q, N)) * np.sqrt(float(g.alpha))
        tn = (t - g._y_train_mean) / g._y_train_std
        vals.append(P.paths_cho(int(g._kind), X, tn, np.array(g._ls), float(g.alpha), omega, phase, w, eps, Xc, g._y_train_mean,
                                g._y_train_std))
    vals = np.array(vals)
    y_std = np.array([g._y_train_std for g in gps])
    idx, _, _, feas, viol = ST.rule(vals, np.array([E2E["LB"]]), np.array([E2E["UB"]]), y_std)
    ok = viol == 0.0
    masked = np.where(ok, vals[0], -INF)
    two = -np.partition(-masked, 1, axis=1)[:, :2]
    value_gap = (two[:, 0] - two[:, 1]) / np.ptp(vals[0], axis=1)
    bound_gap = np.min([np.abs(vals[1] - b).min(axis=1) for b in (E2E["LB"], E2E["UB"]) if np.isfinite(b)], axis=0) / np.ptp(vals[1], axis=1)
    return idx, feas, ok.sum(axis=1), value_gap, bound_gap, vals[0].argmax(axis=1)


def test_suggest_constrained_thompson_picks_the_truths(engine):
    D, M, Q, FEATURES = E2E["D"], E2E["M"], E2E["Q"], E2E["FEATURES"]
    drv, X, y, cv = e2e_driver(engine)
    picks = suggest_constrained_thompson(drv, Q, n_random=M, n_features=FEATURES)
    Xc = engine.get_candidate_rows(np.arange(M), D)
    assert drv._acquisition_function.i == 0 and drv._gp.X_train_.shape[0] == E2E["N"]
    twin, _, _, _ = e2e_driver(engine)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with engine.overlapped_fits():
            twin._gp.fit(twin._space.params, twin._space.target)
            twin._space.constraint.fit(twin._space.params, twin._space._constraint_values)
    rng = twin._random_state
    assert np.array_equal(np.column_stack([rng.uniform(0.0, 1.0, M) for _ in range(D)]), Xc)
    for a, b in zip([drv._gp, drv._space.constraint.model[0]], [twin._gp, twin._space.constraint.model[0]]):
        assert int(a._kind) == int(b._kind) and np.array_equal(a._ls, b._ls)
    want, feas, n_ok, value_gap, bound_gap, free = e2e_truth(twin, X, y, cv, Xc)
    got = B.rows_to_indices(picks, Xc)
    print(f"picks {got.tolist()} truth {want.tolist()} feasible candidates {n_ok.tolist()} value gaps {['%.1e' % g for g in value_gap]} "
          f"bound gaps {['%.1e' % g for g in bound_gap]}")
    assert (n_ok >= 2).all() and (n_ok < M).all(), f"the truth's feasible counts {n_ok.tolist()}: pick another seed"
    assert value_gap.min() >= GAP_FLOOR, f"the truth's own best / second feasible gap {value_gap.min():.2e}: pick another seed"
    assert bound_gap.min() >= GAP_FLOOR, f"the truth's nearest constraint value to its bound {bound_gap.min():.2e}: pick another seed"
    assert not np.array_equal(want, free), "the truth's picks are the unconstrained maximisers: the constraint decides nothing"
    assert np.array_equal(got, want)
    assert B.same_state(drv._random_state, rng)
    # afterwards the models answer for the real data as before
    assert np.array_equal(drv._gp.predict(X[:4]), twin._gp.predict(X[:4]))
    assert np.array_equal(drv._space.constraint.predict(X[:4]), twin._space.constraint.predict(X[:4]))
