"""GPU (-m gpu): log expected improvement (GPBO_ACQ_LOG_EI = 3) at every site that evaluates it — acq_kernel and the ACQ instances of
the selection launch (gpbo_acq_argbest with k_seeds = 2 and >= 3), polish_fused.hip and the host side of the lockstep local search
(gpbo_polish_seeds, gpbo_debug_polish_eval) — against the 50-digit truth of tests/log_ei_truth.py taken on the device's OWN mu / sd
bits, so only the formula is under test; the refusals; and the policy on the real engine.

Bar: |value - truth| <= 8 max(c_ref, 1) eps W, W = 1 + z^2 + |truth| (gradient: (1 + z^2)(|ca dmu| + |cs dsd|)); c_ref = the worst constant
of the formula in NumPy / SciPy (log_ei_truth.reference_values) on the same mu / sd, 8 for the device library's log / erfcx / erfc / exp.

Measured on an MI355X (worst c over the cases; c_ref on the same inputs in brackets; docs/LAB_NOTEBOOK.md section 18):
    acq_kernel = the selection's ACQ instance <4, true> (same bits), M = 2048, eleven y_max      1.14 (1.99); z from -887 690 to 7 356
    the same on the plateau (max mu + 60 s50: every EI zero, EI's pick index 0)                  0.63 (0.63)
    acq_kernel = the ACQ instance <16, true>, M = 2^18 + 1, sample of 2048                       0.94 (1.59)
    small model (N = 25, d = 2), two y_max                                                       1.13 (1.86)
    polish_fused.hip, gpbo_debug_polish_eval, six y_max, z from -25 249 to 1 434                 value 1.08 (1.30), gradient 1.23 (2.71)
    end points of searches from z < -45, gpbo_predict's mu / sd: one launch N = 64 / 300         0.70 / 0.50 (0.50 / 0.44)
                                                                  lockstep N = 64 / 300 / 520    0.50 / 0.44 / 0.47 (the same)
    lockstep host side at end points in every branch of the formula (z 22.9 ... -50)             1.37 (1.22)
    (its first form, plain exp(t * t) * erfc(t), gave 7.2 at z = -7 and 40 at z = -17 there: polish.hip's erfcx_host has the story)
    clipped variances: 36 of 60 candidates on training points, 17 with aa > 0 (-log aa), 19 with +inf; both launch forms the same bits."""
import numpy as np
import pytest

import acq_truth as T
import batch_truth as B
import log_ei_truth as L
import test_gpu_acq_regimes as R
import test_gpu_polish_fused as P
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd import suggest_batch
from oracle import gp_oracle as O
from test_gpu_polish_fused import any_size, lockstep_only  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

XI = R.XI
LOG_EI = 3
TAIL = (40.0, 100.0, 1000.0)


# ---- shared pieces ---------------------------------------------------------------------------------------------------------------
def _neg_truth(tr, mu, sd, y_max):
    """-logEI per candidate as mpf: the truth where it is defined, the convention's value (log(aa), -inf, NaN) elsewhere"""
    conv = L.reference_values(mu, sd, y_max, XI)
    return [-tr["log_ei"][i] if tr["ok"][i] else T._ctx.mpf(-float(conv[i])) for i in range(len(mu))]


def _decided_order(neg, bars, k):
    """(the truth's order of the first k, whether each of the first k gaps exceeds the two bars)"""
    order = L.argbest(neg)[:k + 1]
    return order[:k], all(neg[order[t + 1]] - neg[order[t]] > bars[order[t]] + bars[order[t + 1]] for t in range(k))


def _check_values(site, ys, idx, mu, sd, y_max):
    """the bar over the candidates `idx`; returns (truth, bar, c_dev, c_ref)"""
    tr = L.log_ei_truth(mu[idx], sd[idx], y_max, XI)
    ref = L.reference_values(mu[idx], sd[idx], y_max, XI)
    ok = tr["ok"]
    c_ref = T.worst(T.constants(ref, tr["log_ei"], tr["w"], floor=0.0)[ok])
    bar = 8.0 * max(c_ref, 1.0)                              # fixed before the device's values are looked at
    c = T.constants(-ys[idx], tr["log_ei"], tr["w"], floor=0.0)
    c_dev = T.worst(c[ok])
    print(f"{site} y_max={y_max:+.4f}: c_dev {c_dev:.3f} c_ref {c_ref:.3f} bar {bar:.1f} z [{np.nanmin(tr['z']):.1f}, {np.nanmax(tr['z']):.1f}] "
          f"undefined {int((~ok).sum())}")
    assert np.all(np.isfinite(ys[idx][ok])) and np.all(c[ok] <= bar), (site, y_max, c_dev, bar)
    # sd == 0 / NaN: the convention's value (a logarithm of the device library against NumPy's: to 8 eps of its own scale)
    conv = -1 * ref[~ok]
    got = ys[idx][~ok]
    assert np.array_equal(np.isnan(got), np.isnan(conv)) and np.array_equal(np.isinf(got), np.isinf(conv))
    fin = np.isfinite(conv)
    assert np.array_equal(got[~fin], conv[~fin], equal_nan=True)
    assert np.all(np.abs(got[fin] - conv[fin]) <= 8.0 * T.EPS * (1.0 + np.abs(conv[fin])))
    return tr, bar, c_dev, c_ref


class _Case:
    """test_gpu_acq_regimes.py's recipe (N = 64, d = 2, its NEAR points and its two exact copies of training points) and the device's
    posterior over it, fetched once"""

    def __init__(self, engine, M, sample=None):
        self.X, self.y = R._training()
        self.Xc = R._candidates(M, self.X)
        self.M = M
        self.idx = np.arange(M) if sample is None else sample
        self.ym, self.ysd = R._fit_target(engine, self.X, self.y)
        engine.set_candidates(self.Xc)
        self.mu, self.sd = engine.posterior(0, self.ym, self.ysd)
        s50, hi = float(np.median(self.sd)), float(self.mu.max())
        self.y_maxes = R._sweep(self.mu, self.sd) + [hi + t * s50 for t in TAIL]
        self.plateau = hi + 60.0 * s50

    resident = R._Case.resident


@pytest.fixture(scope="module")
def small(engine):
    return _Case(engine, 2048)


# ---- 1. values across the z range, both launch forms, picks -------------------------------------------------------------------------
@pytest.mark.parametrize("t_index", range(8 + len(TAIL)))
def test_values_and_picks_over_the_z_range(engine, small, t_index):
    small.resident(engine)
    y_max = small.y_maxes[t_index]
    bi, bv, si, sv, ys = R._both_forms(engine, LOG_EI, y_max, k_big=3)          # the same bits in both forms; the picks are NumPy's lexsort
    tr, bar, _, _ = _check_values("argbest M=2048", ys, small.idx, small.mu, small.sd, y_max)
    neg = _neg_truth(tr, small.mu, small.sd, y_max)
    bars = [bar * T.EPS * w if o else 0 for w, o in zip(tr["w"], tr["ok"])]
    order, decided = _decided_order(neg, bars, 1)
    assert decided, "the truth's best / second gap is inside the bar: pick another candidate seed"
    assert bi == order[0]
    if t_index >= 9:
        assert np.nanmax(tr["z"]) < -38.5                   # the whole set is under EI's underflow edge


# ---- 2. the plateau ------------------------------------------------------------------------------------------------------------------
def test_where_ei_is_a_plateau_of_zeros_log_ei_answers(engine, small):
    small.resident(engine)
    y_max = small.plateau
    bi, bv, si, sv, ys = R._both_forms(engine, O.EI, y_max, k_big=3)
    assert bi == 0 and bv == 0.0 and np.all(ys == 0.0) and np.array_equal(si, [0, 1, 2])      # today's behaviour, for the contrast
    bi, bv, si, sv, ys = R._both_forms(engine, LOG_EI, y_max, k_big=3)
    tr, bar, _, _ = _check_values("plateau", ys, small.idx, small.mu, small.sd, y_max)
    neg = _neg_truth(tr, small.mu, small.sd, y_max)
    bars = [bar * T.EPS * w if o else 0 for w, o in zip(tr["w"], tr["ok"])]
    order, decided = _decided_order(neg, bars, 3)
    assert decided
    assert bi == order[0] != 0 and np.array_equal(si, order) and np.isfinite(bv)


# ---- 3. the multi-workgroup selection ------------------------------------------------------------------------------------------------
def test_two_to_the_eighteen_plus_one(engine):
    M = (1 << 18) + 1
    sample = np.unique(np.concatenate([np.arange(90, 160), [0, 5, M - 7, M - 1, 1 << 18], np.random.RandomState(9).randint(0, M, 1980)]))[:2048]
    case = _Case(engine, M, sample=sample)
    y_max = case.y_maxes[6]                                  # max(mu) + 10 median(sd)
    bi, bv, si, sv, ys = R._both_forms(engine, LOG_EI, y_max, k_big=10)
    _check_values("argbest M=2^18+1", ys, case.idx, case.mu, case.sd, y_max)
    assert np.isfinite(ys[np.isfinite(case.mu) & (case.sd > 0)]).all()


# ---- 4. a small model (the one-launch small step's sizes) -----------------------------------------------------------------------------
def test_a_small_model(engine):
    from test_gpu_fused_small import CASES, problem

    N, d, kernel, per_dim, _ = CASES[1]                      # N = 25, d = 2
    X, yn, ls, Xc = problem(N, d, 1000 + N, per_dim)
    engine.fit(X, yn, kernel, ls, 1e-6, slot=0)
    engine.set_candidates(Xc[:2048])
    mu, sd = engine.posterior(0, 0.3, 1.7)
    for y_max in (float(np.median(mu)), float(mu.max()) + 50.0 * float(np.median(sd))):
        bi, bv, si, sv, ys = R._both_forms(engine, LOG_EI, y_max, k_big=3)
        _check_values("small model", ys, np.arange(2048), mu, sd, y_max)


# ---- 5. conventions --------------------------------------------------------------------------------------------------------------------
def test_clipped_variances_and_a_nan_candidate(engine):
    X, y = R._training()
    yn, ym, ysd = O.normalize_targets(y)
    engine.fit(X, yn, O.MATERN25, R.LS, 0.0, slot=0)         # no noise: the variance AT a training point is rounding, clipped at 0 when negative
    Xc = np.vstack([X[:60], np.random.RandomState(3).uniform(size=(4, 2))])
    Xc[9] = np.nan
    engine.set_candidates(Xc)
    mu, sd = engine.posterior(0, ym, ysd)
    y_max = float(np.median(y))
    clipped = sd == 0.0
    aa = mu - y_max - XI
    print(f"clipped {int(clipped.sum())}/60: aa > 0 {int((clipped & (aa > 0)).sum())}, aa <= 0 {int((clipped & (aa <= 0)).sum())}")
    assert (clipped & (aa > 0)).any() and (clipped & (aa <= 0)).any() and np.isnan(mu[9])
    a = engine.acq_argbest(LOG_EI, XI, y_max, k_seeds=2, return_values=True)
    b = engine.acq_argbest(LOG_EI, XI, y_max, k_seeds=64, return_values=True)
    assert np.array_equal(R._bits(a[4]), R._bits(b[4]))
    R._check_picks(a, 2)
    R._check_picks(b, 64)
    ys = b[4]
    assert np.all(ys[clipped & (aa <= 0)] == np.inf)
    pos = clipped & (aa > 0)
    assert np.all(np.abs(ys[pos] + np.log(aa[pos])) <= 8.0 * T.EPS * (1.0 + np.abs(np.log(aa[pos]))))
    assert np.isnan(ys[9]) and b[0] == 9 and np.isnan(b[1])           # the NaN candidate is the arg-best, as numpy's argmin ...
    assert b[2][-1] == 9 and np.isnan(b[3][-1])                       # ... and the last of the sorted seeds
    n_inf = int(np.isinf(ys).sum())
    assert np.all(np.isinf(b[3][-1 - n_inf:-1])) and np.all(np.isfinite(b[3][:-1 - n_inf]))     # +inf after every finite value
    _check_values("conventions", ys, np.arange(64), mu, sd, y_max)


# ---- 6. local search -------------------------------------------------------------------------------------------------------------------
def test_polish_eval_values_and_gradients(debug_engine, any_size):
    eng = debug_engine
    X, y, ls = P._problem(300, 4, 3)
    ym, ys = P._fit(eng, X, y, O.MATERN25, ls)
    wide = np.vstack([np.random.RandomState(6).uniform(size=(52, 4)), X[:12] + 10.0 ** np.linspace(-5, -2, 12)[:, None]])
    first = P._polish_eval(eng, O.UCB, 1.0, 0.0, ym, ys, wide)
    s50, hi = float(np.median(first["sd"])), float(first["mu"].max())
    z_seen, worst = [], [0.0, 0.0, 0.0, 0.0]
    for y_max in (float(np.quantile(first["mu"], 0.25)), float(np.median(first["mu"])), hi + 2 * s50, hi + 10 * s50, hi + 45 * s50, hi + 200 * s50):
        got = P._polish_eval(eng, LOG_EI, XI, y_max, ym, ys, wide)
        assert np.array_equal(got["mu"], first["mu"]) and np.array_equal(got["sd"], first["sd"])
        tr = L.log_ei_truth(got["mu"], got["sd"], y_max, XI, got["dmu"], got["dsd"])
        assert tr["ok"].all()
        ref_f, ref_g = L.reference_values(got["mu"], got["sd"], y_max, XI, got["dmu"], got["dsd"])
        c_ref_f = T.worst(T.constants(ref_f, tr["log_ei"], tr["w"], floor=0.0))
        c_ref_g = T.worst(T.constants(ref_g, tr["g"], tr["w_g"], floor=0.0))
        c_f = T.worst(T.constants(-got["f"], tr["log_ei"], tr["w"], floor=0.0))
        c_g = T.worst(T.constants(got["g"], tr["g"], tr["w_g"], floor=0.0))
        print(f"polish eval y_max={y_max:+.3f}: f c_dev {c_f:.3f} c_ref {c_ref_f:.3f}; g c_dev {c_g:.3f} c_ref {c_ref_g:.3f}; "
              f"z [{tr['z'].min():.1f}, {tr['z'].max():.1f}]")
        worst = [max(a, b) for a, b in zip(worst, (c_f, c_ref_f, c_g, c_ref_g))]
        assert c_f <= 8.0 * max(c_ref_f, 1.0) and c_g <= 8.0 * max(c_ref_g, 1.0)
        z_seen.append(tr["z"])
    print("polish eval worst: f c_dev %.3f c_ref %.3f; g c_dev %.3f c_ref %.3f" % tuple(worst))
    z_seen = np.concatenate(z_seen)
    assert z_seen.min() <= -200.0 and z_seen.max() >= 3.0
    assert all(np.sum((z_seen >= a) & (z_seen < b)) >= 8 for a, b in ((-200, -45), (-45, -28), (-28, -8), (-8, -1), (-1, 3)))


def _oracle_knows_log_ei(monkeypatch):
    """test_gpu_polish_fused._same_or_better asks the oracle for -acq at the returned points: teach it kind 3 (the formula's restatement)"""
    stock = O.base_acq

    def base_acq(kind, mean, std, param, y_max=0.0):
        return L.reference_values(mean, std, y_max, param) if kind == LOG_EI else stock(kind, mean, std, param, y_max)

    monkeypatch.setattr(O, "base_acq", base_acq)


@pytest.mark.parametrize("N,d,ls", [(64, 2, 0.1), (300, 3, 0.12), (520, 3, 0.1)], ids=["one-launch-64", "one-launch-300", "lockstep-520"])
def test_local_searches_leave_the_plateau(debug_engine, lockstep_only, any_size, monkeypatch, N, d, ls):
    """Seeds with z < -45: EI is 0 with a zero gradient there and its runs return their seeds; every log-EI run descends, and its value
    is -truth at the point it returns (mu, sd from gpbo_predict there).  N = 520 (NP = 576 > 512) is served by the lockstep path alone."""
    _oracle_knows_log_ei(monkeypatch)
    eng = debug_engine
    X, y, _ = P._problem(N, d, 40 + N)
    ym, ys = P._fit(eng, X, y, O.MATERN25, ls)
    gp = O.fit_fixed_theta(O.MATERN25, X, y, ls, 1e-6)
    box = np.array([[0.0, 1.0]] * d)
    seeds = np.random.RandomState(12).uniform(0.05, 0.95, size=(10, d))
    mu0, sd0 = eng.predict(seeds, slot=0, y_mean=ym, y_std=ys)
    y_max = float(np.max(mu0 + 50.0 * sd0))
    z0 = (mu0 - y_max - XI) / sd0
    assert np.all(z0 < -45.0)
    f_seed = -1 * L.reference_values(mu0, sd0, y_max, XI)
    ref_ei, _, got_ei, _ = P._both(eng, lockstep_only, O.EI, XI, y_max, ym, ys, seeds, box)
    for res in (ref_ei, got_ei):                            # the contrast: EI's runs stay where they started, at a value of zero
        assert np.array_equal(res[0], seeds) and np.all(res[1] == 0.0)
    ref, rc, got, gc = P._both(eng, lockstep_only, LOG_EI, XI, y_max, ym, ys, seeds, box)
    for name, res in (("lockstep", ref), ("one launch" if N < 520 else "lockstep again", got)):
        x, f, status = res[0], res[1], res[2]
        assert np.all(np.isfinite(f)) and np.all(f < f_seed), (name, f, f_seed)
        assert np.all(x >= 0.0) and np.all(x <= 1.0)
        mu, sd = eng.predict(x, slot=0, y_mean=ym, y_std=ys)
        tr = L.log_ei_truth(mu, sd, y_max, XI)
        c_ref = T.worst(T.constants(L.reference_values(mu, sd, y_max, XI), tr["log_ei"], tr["w"], floor=0.0))
        c = T.constants(-f, tr["log_ei"], tr["w"], floor=0.0)
        print(f"polish N={N} {name}: f_seed [{f_seed.min():.1f}, {f_seed.max():.1f}] f_out [{f.min():.3f}, {f.max():.3f}] z_out "
              f"[{tr['z'].min():.2f}, {tr['z'].max():.2f}] status {status.tolist()} c_dev {T.worst(c):.3f} c_ref {c_ref:.3f}")
        assert tr["ok"].all() and np.all(c <= 8.0 * max(c_ref, 1.0)), (name, T.worst(c))
    P._same_or_better(ref, got, gp, LOG_EI, XI, y_max)
    if N == 520:
        assert all(np.array_equal(a, b) for a, b in zip(ref[:3], got[:3]))


def test_lockstep_end_points_in_every_branch_of_the_formula(debug_engine, lockstep_only, any_size):
    """The host side of the lockstep path has no single-evaluation entry: its formula (std::erfc / std::exp, exp(t^2) erfc(t) for erfcx) is
    read off the values its searches return, at end points with z above -1, between -28 and -1 and below -28.  mu, sd at the end points come
    from gpbo_predict_grad, whose kernels the lockstep rounds run: near z = 0 the weight W is ~2 and leaves no room for another route's sums."""
    eng = debug_engine
    X, y, _ = P._problem(64, 2, 104)
    ym, ys = P._fit(eng, X, y, O.MATERN25, 0.1)
    box = np.array([[0.0, 1.0]] * 2)
    seeds = np.random.RandomState(12).uniform(0.05, 0.95, size=(10, 2))
    mu0, sd0 = eng.predict(seeds, slot=0, y_mean=ym, y_std=ys)
    s50, hi = float(np.median(sd0)), float(mu0.max())
    z_seen, worst = [], [0.0, 0.0]
    lockstep_only(True)
    for y_max in (float(np.min(y)), float(np.median(y)), float(np.max(y)), hi + 3 * s50, hi + 8 * s50, hi + 20 * s50, hi + 50 * s50):
        x, f, status, _ = eng.polish_seeds(LOG_EI, XI, y_max, None, None, [ym], [ys], seeds, box)
        mu, sd = eng.predict_grad(x, slot=0, y_mean=ym, y_std=ys)[:2]
        tr = L.log_ei_truth(mu, sd, y_max, XI)
        c_ref = T.worst(T.constants(L.reference_values(mu, sd, y_max, XI), tr["log_ei"], tr["w"], floor=0.0))
        c = T.constants(-f, tr["log_ei"], tr["w"], floor=0.0)
        print(f"lockstep end points y_max={y_max:+.3f}: c_dev {T.worst(c):.3f} c_ref {c_ref:.3f} z_out [{tr['z'].min():.2f}, {tr['z'].max():.2f}]")
        worst = [max(worst[0], T.worst(c)), max(worst[1], c_ref)]
        assert tr["ok"].all() and np.all(c <= 8.0 * max(c_ref, 1.0)), (y_max, T.worst(c))
        z_seen.append(tr["z"])
    print("lockstep end points worst: c_dev %.3f c_ref %.3f" % tuple(worst))
    z_seen = np.concatenate(z_seen)
    assert np.sum(z_seen > -1.0) >= 5 and np.sum((z_seen <= -1.0) & (z_seen > -28.0)) >= 5 and np.sum(z_seen <= -28.0) >= 5


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals(engine, small):
    small.resident(engine)
    y_max = small.y_maxes[5]
    with pytest.raises(ValueError, match="takes no constraints"):
        engine.acq_argbest(LOG_EI, XI, y_max, [-np.inf], [0.5], k_seeds=3)
    seeds = np.random.RandomState(1).uniform(size=(4, 2))
    box = np.array([[0.0, 1.0]] * 2)
    with pytest.raises(ValueError, match="takes no constraints"):
        engine.polish_seeds(LOG_EI, XI, y_max, [-np.inf], [0.5], [small.ym, 0.0], [small.ysd, 1.0], seeds, box)
    with pytest.raises(ValueError, match="GPBO_ACQ_LOG_EI"):
        engine.evolve_mixed(LOG_EI, XI, y_max, small.ym, small.ysd, [(0, 0, 1), (1, 1, 1)], np.array([[0.0, 1.0], [0.0, 5.0]]),
                            np.random.RandomState(2).uniform(size=(30, 2)), np.random.RandomState(3))
    for call in (lambda: engine.acq_argbest(4, XI, y_max, k_seeds=3),
                 lambda: engine.polish_seeds(4, XI, y_max, None, None, [small.ym], [small.ysd], seeds, box)):
        with pytest.raises(ValueError, match="unknown acquisition"):
            call()
    small.resident(engine)                                  # the refused calls changed nothing
    assert engine.acq_argbest(LOG_EI, XI, y_max, k_seeds=0)[0] >= 0


# ---- 8. the seam -------------------------------------------------------------------------------------------------------------------------
D, M = 3, 2000
BOUNDS = np.array([[0.0, 1.0]] * D)


def _driver(engine, N=40, **kw):
    X = np.random.RandomState(100 + N).uniform(size=(N, D))
    y = np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1]) + X[:, 2] ** 2
    return B.Driver(engine, X, y, BOUNDS, A.LogExpectedImprovement(), seed=7, n_random=M, **kw), X, y


def test_the_policy_on_the_engine(engine):
    drv, X, y = _driver(engine)
    fn, gp = drv._acquisition_function, drv._gp
    x = drv.suggest_first()
    Xc = engine.get_candidate_rows(np.arange(M), D)
    mu, sd = engine.posterior(0, float(gp._y_train_mean), float(gp._y_train_std))
    tr = L.log_ei_truth(mu, sd, fn.y_max, fn.xi)
    neg = _neg_truth(tr, mu, sd, fn.y_max)
    order, decided = _decided_order(neg, [8.0 * T.EPS * w if o else 0 for w, o in zip(tr["w"], tr["ok"])], 1)
    assert decided, "the truth's best / second gap is inside the bar: pick another seed"
    assert fn.y_max == float(y.max()) and B.rows_to_indices([x], Xc)[0] == order[0]
    # with local searches: the same candidates (a twin on the same RandomState seed), a point at least as good
    twin, _, _ = _driver(engine)
    x2 = twin._acquisition_function.suggest(gp=twin._gp, target_space=twin._space, n_random=M, n_smart=10, fit_gp=True,
                                            random_state=twin._random_state)
    objective = twin._acquisition_function._get_acq(gp=twin._gp)
    f_pick, f_smart = float(objective(x)[0]), float(objective(x2)[0])
    print(f"seam: -logEI at the random stage's pick {f_pick:.6f}, after the local searches {f_smart:.6f}")
    assert np.all(x2 >= 0.0) and np.all(x2 <= 1.0) and f_smart <= f_pick


def test_suggest_batch_on_the_engine(engine):
    drv, X, y = _driver(engine, n_restarts_optimizer=0)
    drv.suggest_first()
    Xq = np.random.RandomState(9).uniform(size=(64, D))
    mu0, sd0 = drv._gp.predict(Xq, return_std=True)
    picks = suggest_batch(drv, 3)
    Xc = engine.get_candidate_rows(np.arange(M), D)
    assert len(picks) == 3 and len(set(B.rows_to_indices(picks, Xc).tolist())) == 3
    mu1, sd1 = drv._gp.predict(Xq, return_std=True)
    assert np.array_equal(mu0, mu1) and np.array_equal(sd0, sd1)
