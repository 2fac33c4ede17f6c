"""GPU (-m gpu): the acquisition value and the pick made from it over the WHOLE z range — both tails, the erf / erfc switch at |z| = 1,
the upper reflection, the underflow edge at |z| ~ 38.5 and the two plateaus the formula really produces — through the product's
gpbo_acq_argbest, in both launch forms (k_seeds = 2: acq_kernel + the passes; k_seeds = 3: the ACQ instances of the selection launch),
against the 50-digit truth of tests/acq_truth.py taken on the device's OWN mu / sd bits, so only the formula is under test.

Late in a real run y_max sits above nearly every posterior mean: every EI / POI value is in the lower tail and the arg-best is decided
among values of 1e-20 ... 1e-300.  The parity tests' bar (1e-9 of the batch's largest value) would pass a kernel returning zeros there.

Bar: |ys + truth| <= 8 c_ref eps (1 + z^2) T + DBL_MIN, c_ref = the worst constant of SciPy's arithmetic on the same mu / sd (~1-2; 8 for
the device library's erf / erfc / exp, specified to a few ulp where Cephes measures about one).

Measured on an MI355X (c = worst constant over the sweep; SciPy's on the same mu / sd in brackets; docs/LAB_NOTEBOOK.md section 16):
    M = 2048, eight y_max     EI  c = 1.44 (1.43)      POI  c = 1.11 (1.85)      under the DBL_MIN floor: 3.2 % of the pairs
    M = 2^18 + 1, three       EI  c = 1.51 (1.53)      POI  c = 1.08 (1.87)      (sample of 2048 indices)
    seven constraints         factors c = 1.07, 0.32, 0.70, 0.008, 0 (exactly 1), 1.02, 0.93 (reference's worst 2.01); the product
                              uses 0.0005 of its bar — the same-tail band's W ~ 2 (1 + z^2) against a factor of ~1e-6 makes that bar wide,
                              so the factors' own constants are asserted too
    subnormal results are KEPT (every value whose T lies in 1e-320 ... DBL_MIN came back non-zero: 12/12, 14/14): recorded, not asserted;
    both launch forms give the same bits everywhere, plateaus included."""
import numpy as np
import pytest

import acq_truth as T
from bayesianoptimization_amd import _lib
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

XI = 0.01
N_TRAIN, DIM, LS, NOISE = 64, 2, 0.05, 1e-6
BINS = [-38.5, -20.0, -8.0, -2.0, -1.0, 1.0, 2.0, 8.0, 38.5]
NEAR = 48


def _training():
    rng = np.random.RandomState(7)
    X = rng.uniform(size=(N_TRAIN, DIM))
    y = np.sin(3 * X.sum(1)) + 0.05 * rng.randn(N_TRAIN)
    return X, y


def _candidates(M, X):
    """uniform points, NEAR points 1e-6 ... 1e-2 from training points (small sd, large |z|), two exact copies of training points"""
    rng = np.random.RandomState(8)
    Xc = rng.uniform(size=(M, DIM))
    r = 10.0 ** rng.uniform(-6.0, -2.0, NEAR)
    u = rng.standard_normal((NEAR, DIM))
    Xc[100:100 + NEAR] = X[rng.randint(0, N_TRAIN, NEAR)] + r[:, None] * u / np.linalg.norm(u, axis=1)[:, None]
    Xc[5], Xc[M - 7] = X[3], X[40]
    return Xc


def _sweep(mu, sd):
    """y_max values from the fetched posterior: far below every mean (upper tail, reflection), inside the means' range (|z| ~ 1), and
    above every mean by 1 ... 20 typical sd (lower tail down to the underflow edge: the late-run regime)"""
    s50, lo, hi = float(np.median(sd)), float(mu.min()), float(mu.max())
    return [lo - 5 * s50, float(np.quantile(mu, 0.1)), float(np.median(mu)), float(np.quantile(mu, 0.9)), hi + s50, hi + 4 * s50,
            hi + 10 * s50, hi + 20 * s50]


def _fit_target(engine, X, y):
    yn, ym, ysd = O.normalize_targets(y)
    engine.fit(X, yn, O.MATERN25, LS, NOISE, slot=0)
    return ym, ysd


class _Case:
    """the device's posterior over one candidate set, and the truth per y_max (computed once, shared, never written to)"""

    def __init__(self, engine, M, sample=None, sweep=None):
        self.X, self.y = _training()
        self.Xc = _candidates(M, self.X)
        self.M = M
        self.idx = np.arange(M) if sample is None else sample
        self.ym, self.ysd = _fit_target(engine, self.X, self.y)
        engine.set_candidates(self.Xc)
        self.mu, self.sd = engine.posterior(0, self.ym, self.ysd)
        self.y_maxes = _sweep(self.mu, self.sd) if sweep is None else sweep(self.mu, self.sd)
        self.truth = [T.acq_truth(self.mu[self.idx], self.sd[self.idx], ymx, XI) for ymx in self.y_maxes]

    def resident(self, engine):
        """(the session's engine serves other tests in between: put this case's model, candidates and posterior back)"""
        _fit_target(engine, self.X, self.y)
        engine.set_candidates(self.Xc)
        mu, sd = engine.posterior(0, self.ym, self.ysd)
        assert np.array_equal(mu, self.mu, equal_nan=True) and np.array_equal(sd, self.sd, equal_nan=True)


@pytest.fixture(scope="module")
def small(engine):
    return _Case(engine, 2048)


@pytest.fixture(scope="module")
def big(engine):
    M = (1 << 18) + 1
    sample = np.unique(np.concatenate([np.arange(90, 160), [0, 5, M - 7, M - 1, 1 << 18], np.random.RandomState(9).randint(0, M, 1980)]))[:2048]
    return _Case(engine, M, sample=sample, sweep=lambda mu, sd: [_sweep(mu, sd)[i] for i in (2, 5, 6)])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _lexsort_picks(ys, k):
    nan = np.isnan(ys)
    return np.lexsort((np.arange(ys.shape[0]), np.where(nan, np.inf, np.where(ys == 0.0, 0.0, ys)), nan))[:k]


def _check_picks(res, k):
    """the arg-best and the seeds are NumPy's argmin / argsort[:k] of the returned values, ties to the lowest index"""
    bi, bv, si, sv, ys = res
    want = _lexsort_picks(ys, k)
    assert np.array_equal(si, want)
    assert np.array_equal(_bits(sv), _bits(ys[si]))
    nan = np.isnan(ys)
    if nan.any():
        assert bi == int(np.flatnonzero(nan)[0]) and np.isnan(bv)
    else:
        assert bi == want[0] and _bits([bv])[0] == _bits(ys[bi:bi + 1])[0]
        assert ys[bi] == ys.min()


def _both_forms(engine, acq, y_max, lb=None, ub=None, k_big=3):
    """k_seeds = 2 (acq_kernel + the pass form) and k_seeds >= 3 (values made inside the selection launch): the same bits"""
    a = engine.acq_argbest(acq, XI, y_max, lb, ub, k_seeds=2, return_values=True)
    b = engine.acq_argbest(acq, XI, y_max, lb, ub, k_seeds=k_big, return_values=True)
    assert np.array_equal(_bits(a[4]), _bits(b[4]))
    assert a[0] == b[0] and _bits([a[1]])[0] == _bits([b[1]])[0]
    assert np.array_equal(a[2], b[2][:2]) and np.array_equal(_bits(a[3]), _bits(b[3][:2]))
    _check_picks(a, 2)
    _check_picks(b, k_big)
    return b


def _decided(neg_truth, bars):
    """(argmin of the truth, whether its top-2 gap exceeds twice the bar at those two candidates)"""
    order = sorted(range(len(neg_truth)), key=lambda i: (neg_truth[i], i))[:2]
    i0, i1 = order
    return i0, (neg_truth[i1] - neg_truth[i0]) > 2 * max(bars[i0], bars[i1])


def _run_sweep(engine, case, acq, k_big):
    name = "ei" if acq == O.EI else "poi"
    case.resident(engine)
    idx = case.idx
    c_dev, c_ref, floor_pairs, pairs, decided, z_all, sub = [], [], 0, 0, [], [], [0, 0]
    with np.errstate(all="ignore"):
        refs = [T.reference_values(case.mu[idx], case.sd[idx], ymx, XI)[0 if acq == O.EI else 1] for ymx in case.y_maxes]
    # c_ref first, from SciPy on the same mu / sd (never from the device's values): the bar is fixed before the device is looked at
    for tr, ref in zip(case.truth, refs):
        c_ref.append(T.worst(T.constants(ref, tr[name], tr["w_" + name])))
    bar = 8.0 * max(c_ref)
    for ymx, tr, ref in zip(case.y_maxes, case.truth, refs):
        bi, bv, si, sv, ys = _both_forms(engine, acq, ymx, k_big=k_big)
        ok = tr["ok"]
        got = -ys[idx]
        c = T.constants(got, tr[name], tr["w_" + name])
        c_dev.append(T.worst(c))
        # sd == 0 or a non-finite value: the NumPy formula's own result, signs of zero included
        odd = ~ok | ~np.isfinite(ys[idx])
        assert np.array_equal(ys[idx][odd], -1 * ref[odd], equal_nan=True)
        num = odd & ~np.isnan(ref)
        assert np.array_equal(np.signbit(ys[idx][num]), np.signbit(-1 * ref[num]))
        t = tr["t_" + name][ok]
        floor_pairs += int(np.sum(t < T.DBL_MIN))
        pairs += int(ok.sum())
        z_all.append(tr["z"][ok])
        tiny = (t < T.DBL_MIN) & (t > 1e-320)
        sub[0] += int(tiny.sum())
        sub[1] += int(np.sum(got[ok][tiny] != 0.0))
        print(f"{name} M={case.M} y_max={ymx:+.4f}: c_dev {c_dev[-1]:.3f} c_ref {c_ref[len(c_dev) - 1]:.3f} best {bv:.3e} at {bi} "
              f"z[{np.nanmin(tr['z']):.1f}, {np.nanmax(tr['z']):.1f}] under floor {int(np.sum(t < T.DBL_MIN))}")
        assert np.all(c[ok & np.isfinite(ys[idx])] <= bar), (name, ymx, T.worst(c), bar)
        # the pick, where the truth decides it
        if len(idx) == case.M and ok.all():
            neg = [-v for v in tr[name]]
            bars = [bar * T.EPS * w + T.DBL_MIN for w in tr["w_" + name]]
            i0, dec = _decided(neg, bars)
            decided.append(bool(dec))
            if dec:
                assert bi == i0, (name, ymx)
    print(f"{name} M={case.M}: worst c_dev {max(c_dev):.3f} worst c_ref {max(c_ref):.3f} bar {bar:.2f}; under the floor "
          f"{floor_pairs}/{pairs} = {floor_pairs / pairs:.4f}; results in the subnormal range kept non-zero: {sub[1]}/{sub[0]}")
    assert floor_pairs <= 0.05 * pairs                     # the floor is a condition, not a tolerance: it cannot carry the test
    return np.concatenate(z_all), decided


@pytest.mark.parametrize("acq", [O.EI, O.POI], ids=["ei", "poi"])
def test_values_and_picks_over_the_whole_z_range(engine, small, acq):
    z, decided = _run_sweep(engine, small, acq, k_big=3)
    # the coverage is asserted, so a change to the data cannot hollow the test out
    counts = np.histogram(z, BINS)[0]
    assert np.all(counts >= 50), counts
    assert np.sum(z < BINS[0]) >= 10 and np.sum(z >= BINS[-1]) >= 10
    assert len(decided) == len(small.y_maxes) and sum(decided) >= len(decided) / 2
    if acq == O.EI:
        assert decided[-1] and decided[-2]                  # the deep-tail sweeps: the best EI there is 1e-25 and 1e-80


@pytest.mark.parametrize("acq", [O.EI, O.POI], ids=["ei", "poi"])
def test_plateaus_resolve_to_the_lowest_index(engine, small, acq):
    """POI saturates at exactly -1.0 for every candidate once y_max is far below every mean; EI underflows to -0.0 (aa * 0 = -0, sd * 0
    = +0, their sum +0, negated) once it is far above.  Both are one plateau: index 0 and seeds 0 ... k - 1, as NumPy's argmin."""
    small.resident(engine)
    y_max = float(small.mu.min()) - 100.0 if acq == O.POI else float(small.mu.max()) + 100.0
    with np.errstate(all="ignore"):
        ref = -1 * O.base_acq(acq, small.mu, small.sd, XI, y_max)
    assert np.all(ref == (-1.0 if acq == O.POI else 0.0)) and np.all(np.signbit(ref))
    for k in (3, 10):
        bi, bv, si, sv, ys = _both_forms(engine, acq, y_max, k_big=k)
        assert np.array_equal(_bits(ys), _bits(ref))
        assert bi == 0 and np.array_equal(si, np.arange(k)) and _bits([bv])[0] == _bits(ref[:1])[0]


@pytest.mark.parametrize("acq", [O.EI, O.POI], ids=["ei", "poi"])
def test_the_sixteen_item_instance_at_two_to_the_eighteen_plus_one(engine, big, acq):
    """M = 2^18 + 1: ITEMS switches from 4 to 16 (the ITEMS = 16, ACQ = true instance with k_seeds = 10).  The truth on a fixed sample of
    2048 indices (the near-training points, both ends, the last block's single item); the picks over all of ys."""
    z, _ = _run_sweep(engine, big, acq, k_big=10)
    assert z.min() < -38.5 and z.max() > 38.5 and np.sum(np.abs(z) < 1) >= 50


# ---- constraints at the limit: seven factors (GPBO_MAX_MODELS = 8) -----------------------------------------------------------------
def _constraint_targets(X):
    s = X.sum(1)
    return [np.cos(2 * s), X[:, 0] - X[:, 1], np.sin(5 * X[:, 0]), X[:, 0] * X[:, 1], np.cos(4 * X[:, 1]), s * s, np.sin(3 * s + 1.0)]


LS_C = (0.1, 0.08, 0.06, 0.03, 0.1, 0.05, 0.07)


def test_seven_constraints(engine, small):
    try:
        _seven_constraints(engine, small)
    finally:
        # the session's engine is shared and other tests rely on slots they never fitted being unfitted: a fit that fails (duplicate
        # rows, no noise: not positive definite) leaves its slot unfitted and the context usable (test_not_positive_definite_...)
        dup = np.array([[0.1, 0.2], [0.1, 0.2], [0.5, 0.5]])
        for slot in range(1, 8):
            with pytest.raises(np.linalg.LinAlgError):
                engine.fit(dup, np.zeros(3), O.MATERN25, 1.0, 0.0, slot=slot)
            with pytest.raises(_lib.GpboError):
                engine.posterior(slot, fetch=False)


def _seven_constraints(engine, small):
    X, y = small.X, small.y
    small.resident(engine)
    ms, ss, stds = [], [], []
    for j, (c, ls) in enumerate(zip(_constraint_targets(X), LS_C)):
        cn, cm, cs = O.normalize_targets(c)
        engine.fit(X, cn, O.MATERN25, ls, NOISE, slot=j + 1)
        m, s = engine.posterior(j + 1, cm, cs)
        ms.append(m); ss.append(s); stds.append(cs)
    q = lambda j, p: float(np.quantile(ms[j], p))
    s50 = [float(np.median(s)) for s in ss]
    lb4 = float(ms[3].max()) + 3.0 * s50[3]                 # both ends several sd above the mean: Phi(zu) - Phi(zl) cancels
    lb = [-np.inf, q(1, 0.3), q(2, 0.05), lb4, -np.inf, -np.inf, q(6, 0.2)]
    ub = [q(0, 0.5), np.inf, q(2, 0.95), lb4 + 0.01 * stds[3], np.inf, q(5, 0.02), q(6, 0.7)]
    bands = [T.band_truth(ms[j], ss[j], lb[j], ub[j]) for j in range(7)]
    c_band_ref = max(T.worst(T.constants(T.reference_band(ms[j], ss[j], lb[j], ub[j]), bands[j]["p"], bands[j]["w"])) for j in range(7))
    assert all(p == 1 for p in bands[4]["p"]) and all(b["ok"].all() for b in bands)
    zu4, zl4 = (ub[3] - ms[3]) / ss[3], (lb[3] - ms[3]) / ss[3]
    assert np.mean((zl4 > 2) & (zu4 > 2)) > 0.5            # the same-tail band is one for most candidates
    worst_share, c_band_dev = 0.0, []
    for t_index in (3, 5):                                  # y_max inside the means' range, and above every mean
        y_max, tr = small.y_maxes[t_index], small.truth[t_index]
        with np.errstate(all="ignore"):
            ref_ei = T.reference_values(small.mu, small.sd, y_max, XI)[0]
        bar_ei = 8.0 * T.worst(T.constants(ref_ei, tr["ei"], tr["w_ei"]))
        bar_band = 8.0 * c_band_ref
        # the product's bar = the sum of the factors' relative bars plus EI's, written without dividing by factors that may be 0:
        # prod (|t_i| + b_i) - prod |t_i|
        bi, bv, si, sv, ys = _both_forms(engine, O.EI, y_max, lb, ub, k_big=5)
        truth, hi, lo = [], [], []
        for m in range(small.M):
            terms = [(tr["ei"][m], bar_ei * T.EPS * tr["w_ei"][m])] + [(b["p"][m], bar_band * T.EPS * b["w"][m]) for b in bands]
            t = a = r = 1
            for v, b in terms:
                t, a, r = t * v, a * abs(v), r * (abs(v) + b)
            truth.append(-t); hi.append(r - a + T.DBL_MIN); lo.append(a)
        err = [abs(T._ctx.mpf(float(g)) - t) for g, t in zip(ys, truth)]
        share = max(float(e / h) for e, h in zip(err, hi))
        worst_share = max(worst_share, share)
        under = sum(1 for a in lo if a < T.DBL_MIN)
        print(f"seven constraints y_max={y_max:+.4f}: worst |error| / bar {share:.4f}; bar_ei {bar_ei:.2f} bar_band {bar_band:.2f}; "
              f"best {bv:.3e} at {bi}; products under the floor {under}/{small.M}; pick decided by the truth: {bool(_decided(truth, hi)[1])}")
        assert share <= 1.0
        assert under <= 0.05 * small.M
        i0, dec = _decided(truth, hi)
        if dec:                                             # (the cancelling band's bar is wide: the truth rarely decides here)
            assert bi == i0
    # the device's constant per factor: ys(EI, factor j) = fl(ys(EI) * p_j) with the SAME ys(EI) bits (asserted by _both_forms' bit
    # equality of the unconstrained values), so |ys_j - ys p_j| - half an ulp of the product - DBL_MIN <= |ys| |p_j(device) - p_j|
    y_max = small.y_maxes[3]
    base = engine.acq_argbest(O.EI, XI, y_max, k_seeds=3, return_values=True)[4]
    mpf = T._ctx.mpf
    for j in range(7):                                      # (a single constraint is read from slot 1: put model j there)
        cn, cm, cs = O.normalize_targets(_constraint_targets(X)[j])
        engine.fit(X, cn, O.MATERN25, LS_C[j], NOISE, slot=1)
        m1, s1 = engine.posterior(1, cm, cs)
        assert np.array_equal(m1, ms[j]) and np.array_equal(s1, ss[j])
        one = engine.acq_argbest(O.EI, XI, y_max, [lb[j]], [ub[j]], k_seeds=3, return_values=True)[4]
        cs = [0.0]
        for m in np.flatnonzero(np.abs(base) > 1e-200):
            b, o, w = mpf(float(base[m])), mpf(float(one[m])), bands[j]["w"][m]
            e = abs(o - b * bands[j]["p"][m]) - abs(o) * T.EPS / 2 - T.DBL_MIN
            if e > 0:
                cs.append(float(e / (abs(b) * T.EPS * w)) if w > 0 else np.inf)
        c_band_dev.append(max(cs))
    print(f"factor constants on the device: {[round(c, 3) for c in c_band_dev]}; the reference's worst {c_band_ref:.3f}; "
          f"product: worst |error| / bar {worst_share:.4f}")
    assert c_band_dev[4] == 0.0                             # lb = -inf, ub = +inf: exactly 1
    assert max(c_band_dev) <= 8.0 * c_band_ref
