"""GPU (-m gpu): log constrained expected improvement and log feasibility (GPBO_ACQ_LOG_CEI = 5, GPBO_ACQ_LOG_FEAS = 6) at every site
that evaluates them — acq_kernel<true> and the LOG_SUM instances of the selection launch (gpbo_acq_argbest with k_seeds = 2 and >= 3),
the group form, and the host side of the lockstep local search (gpbo_polish_seeds, gpbo_debug_polish_objective) — against the
50-digit truth of tests/log_cei_truth.py taken on the device's OWN mu / sd bits, so only the formula is under test; the refusals; and
the policy on the real engine.

Bar: |value - truth| <= 8 max(c_ref, 1) eps W with log_cei_truth's derived weights; c_ref = the worst constant of the header's words in
NumPy / SciPy (log_cei_truth.reference_values) on the same mu / sd, 8 for the device library's log / erf / erfc / erfcx / expm1 (the
project's own factor, tests/test_gpu_log_ei.py).

Shapes: test_gpu_log_ei.py's small ones — N = 24, d = 2, M = 2000 (two workgroups of the selection's block stage, the second part
full) and M = 1031 (seven candidates in the second), one constraint in slot 1 and two in slots 1 and 2, fitted at fixed theta.  The
tails are reached by moving y_max and the bounds: the constraint posterior of slot 1 has means in [-1.0, 0.9] and deviations from
0.003 to 0.45, so a bound at 5 is 9 to 2000 sigma away.

Measured on an MI355X (worst c over the cases; c_ref on the same inputs in brackets):
    acq_kernel<true> = the selection's LOG_SUM instance (same bits), M = 2000, twelve bound configurations   kind 5: 1.03 (1.58), kind 6: 0.68 (0.79)
    the same with y_max 60 median deviations above every mean, two configurations                            kind 5: 0.96 (1.23)
    M = 1031, three configurations                                                                           kind 5: 0.96 (1.41), kind 6: 0.51 (0.68)
    the plateau case (GPBO_ACQ_EI with the constraint: zero keys at 100 % of the candidates, arg-best 0)    kind 5: 0.51 (0.51)
    gpbo_debug_polish_objective, 40 points, seven cases, bounds up to 11 711 sigma away                      f 1.23 (1.19), gradient 1.52 (1.97)
    gpbo_polish_seeds from the eight best candidates: every status 0 / 1, 10 - 38 rounds, f below the best candidate's key."""
import numpy as np
import pytest

import acq_truth as T
import batch_truth as B
import log_cei_truth as C
import log_ei_truth as L
import test_gpu_acq_regimes as R
from bayesianoptimization_amd import _lib
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd.constraint_model import HipConstraintModel
from bayesianoptimization_amd.engine import GroupEngine
from bayesianoptimization_amd.float_space import FloatSpace
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

XI = 0.01
LOG_EI, LOG_CEI, LOG_FEAS = 3, 5, 6
INF = np.inf

#: name -> (lb, ub) of slots 1.. : lb-only, ub-only and two-sided; bands that contain the constraint posterior, bands ~5 and >= 30 sigma
#: away from it, a narrow band in a tail; two constraints
CONFIGS = {
    "lb-contains": ([-0.2], [INF]), "lb-5-sigma": ([1.5], [INF]), "lb-30-sigma": ([5.0], [INF]),
    "ub-contains": ([-INF], [0.3]), "ub-5-sigma": ([-INF], [-1.5]), "ub-30-sigma": ([-INF], [-5.0]),
    "two-contains": ([-0.5], [0.5]), "two-5-sigma": ([1.0], [1.2]), "two-30-sigma": ([3.0], [3.5]),
    "two-narrow-in-a-tail": ([2.0], [2.0 + 1e-6]),
    "two-constraints": ([-0.5, 0.9], [0.5, INF]), "two-constraints-far": ([1.0, -INF], [1.2, -0.6]),
}


class _Case:
    """log_cei_truth.small_problem on the engine: slots 0, 1, 2 fitted at fixed theta, the candidates resident, the device's posteriors
    fetched once"""

    def __init__(self, engine, M):
        self.X, y, c1, c2, self.Xc = C.small_problem(M)
        self.M = M
        self.norm = [O.normalize_targets(t) for t in (y, c1, c2)]            # (normalised targets, mean, std) per slot
        self.y_max = float(y.max())
        self.post = self.resident(engine, fetch=True)

    def fit(self, engine):
        for slot, (tn, _, _) in enumerate(self.norm):
            engine.fit(self.X, tn, O.MATERN25, C.SMALL_LS, C.SMALL_NOISE, slot=slot)

    def resident(self, engine, fetch=False, Xc=None):
        self.fit(engine)
        engine.set_candidates(self.Xc if Xc is None else Xc)
        return [engine.posterior(slot, m, s, fetch=fetch) for slot, (_, m, s) in enumerate(self.norm)]

    def cons(self, lb, ub, post=None, idx=slice(None)):
        post = self.post if post is None else post
        return [(float(lb[j]), float(ub[j]), post[j + 1][0][idx], post[j + 1][1][idx]) for j in range(len(lb))]

    y_means = property(lambda self: [m for _, m, _ in self.norm])
    y_stds = property(lambda self: [s for _, _, s in self.norm])


@pytest.fixture(scope="module")
def small(engine):
    return _Case(engine, C.SMALL_M)


@pytest.fixture(scope="module")
def odd(engine):
    return _Case(engine, 1031)


def _both_forms(engine, acq, y_max, lb, ub, k_big=3):
    """k_seeds = 2 (acq_kernel + the pass form) and k_seeds >= 3 (values made inside the selection launch): the same bits; the picks are
    NumPy's lexsort of the returned values"""
    a = engine.acq_argbest(acq, XI, y_max, lb, ub, k_seeds=2, return_values=True)
    b = engine.acq_argbest(acq, XI, y_max, lb, ub, k_seeds=k_big, return_values=True)
    assert np.array_equal(R._bits(a[4]), R._bits(b[4]))
    assert a[0] == b[0] and R._bits([a[1]])[0] == R._bits([b[1]])[0]
    assert np.array_equal(a[2], b[2][:2]) and np.array_equal(R._bits(a[3]), R._bits(b[3][:2]))
    R._check_picks(a, 2)
    R._check_picks(b, k_big)
    return b


def _truth(case, lb, ub, y_max):
    """the truth of kinds 5 and 6 on the case's fetched posteriors; the log EI part is taken once per (case, y_max)"""
    held = case.__dict__.setdefault("_log_ei", {})
    if y_max not in held:
        held[y_max] = L.log_ei_truth(case.post[0][0], case.post[0][1], y_max, XI)
    tr = C.log_cei_truth(LOG_CEI, case.post[0][0], case.post[0][1], y_max, XI, case.cons(lb, ub), ei=held[y_max])
    assert tr["ok"].all()
    return tr


def _check(site, kind, res, case, lb, ub, y_max, tr, k):
    """values to the bar, the arg-best and the top k in the truth's order as far as the truth decides it; returns (c_dev, c_ref)"""
    bi, bv, si, sv, ys = res
    key, w = (tr["key"], tr["w"]) if kind == LOG_CEI else (tr["key_feas"], tr["w_feas"])
    ref = C.reference_values(kind, case.post[0][0], case.post[0][1], y_max, XI, case.cons(lb, ub))
    c_ref = T.worst(T.constants(ref, key, w, floor=0.0))
    bar = 8.0 * max(c_ref, 1.0)                              # fixed before the device's values are looked at
    c = T.constants(ys, key, w, floor=0.0)
    c_dev = T.worst(c)
    print(f"{site} kind {kind}: c_dev {c_dev:.3f} c_ref {c_ref:.3f} bar {bar:.1f} keys [{float(min(key)):.4g}, {float(max(key)):.4g}]")
    assert np.isfinite(ys).all() and np.all(c <= bar), (site, kind, c_dev, bar)
    bars = [bar * T.EPS * v for v in w]
    order = C.argbest(list(key))[:k + 1]
    decided = 0
    while decided < k and key[order[decided + 1]] - key[order[decided]] > bars[order[decided]] + bars[order[decided + 1]]:
        decided += 1
    if decided >= 1:
        assert bi == order[0] and np.array_equal(si[:decided], order[:decided])
    else:      # (a band that contains nearly every posterior: log p = -0 many times over) the pick is within the bars of the truth's best
        assert key[bi] - key[order[0]] <= bars[bi] + bars[order[0]]
    return c_dev, c_ref


# ---- 1. values, both launch forms, picks ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_values_and_picks(engine, small, name):
    lb, ub = CONFIGS[name]
    small.resident(engine)
    tr = _truth(small, lb, ub, small.y_max)
    for kind in (LOG_CEI, LOG_FEAS):
        res = _both_forms(engine, kind, small.y_max, lb, ub, k_big=3)
        _check(name, kind, res, small, lb, ub, small.y_max, tr, 3)


@pytest.mark.parametrize("name", ["two-30-sigma", "two-constraints"])
def test_values_where_log_ei_is_in_its_tail_too(engine, small, name):
    """y_max 60 median deviations above every mean: log EI runs in its erfcx and series branches, and EI itself is zero at most candidates"""
    lb, ub = CONFIGS[name]
    small.resident(engine)
    mu, sd = small.post[0]
    y_max = float(mu.max()) + 60.0 * float(np.median(sd))
    tr = _truth(small, lb, ub, y_max)
    res = _both_forms(engine, LOG_CEI, y_max, lb, ub, k_big=10)
    _check(name + " tail", LOG_CEI, res, small, lb, ub, y_max, tr, 10)


@pytest.mark.parametrize("name", ["two-contains", "lb-30-sigma", "two-constraints"])
def test_an_m_with_seven_candidates_in_the_last_workgroup(engine, odd, name):
    lb, ub = CONFIGS[name]
    odd.resident(engine)
    tr = _truth(odd, lb, ub, odd.y_max)
    for kind in (LOG_CEI, LOG_FEAS):
        res = _both_forms(engine, kind, odd.y_max, lb, ub, k_big=5)
        assert res[4].shape == (1031,)
        _check(name + " M=1031", kind, res, odd, lb, ub, odd.y_max, tr, 5)


# ---- 2. without a constraint: GPBO_ACQ_LOG_EI's bits --------------------------------------------------------------------------------------
def test_kind_five_without_a_constraint_is_log_ei(engine, small):
    small.resident(engine)
    for y_max in (small.y_max, small.y_max + 30.0):
        for k in (2, 8):
            a = engine.acq_argbest(LOG_EI, XI, y_max, k_seeds=k, return_values=True)
            b = engine.acq_argbest(LOG_CEI, XI, y_max, k_seeds=k, return_values=True)
            assert a[0] == b[0] and R._bits([a[1]])[0] == R._bits([b[1]])[0]
            assert np.array_equal(a[2], b[2]) and np.array_equal(R._bits(a[3]), R._bits(b[3])) and np.array_equal(R._bits(a[4]), R._bits(b[4]))


# ---- 3. the reason to exist ----------------------------------------------------------------------------------------------------------------
def test_where_the_constrained_product_is_a_plateau_of_zeros_kind_five_answers(engine, small):
    """the case whose condition tests/test_log_cei_host.py checks on the reference alone"""
    lb, ub = [C.PLATEAU_LB], [C.PLATEAU_UB]
    small.resident(engine)
    bi, bv, si, sv, ys = _both_forms(engine, O.EI, small.y_max, lb, ub, k_big=3)
    share = float(np.mean(ys == 0.0))
    print(f"GPBO_ACQ_EI with the constraint: {share:.1%} zero keys, arg-best {bi}")
    assert share >= 0.90
    if share == 1.0:
        assert bi == 0 and np.array_equal(si, [0, 1, 2])     # the plateau: candidate 0, whatever it is
    tr = _truth(small, lb, ub, small.y_max)
    res = _both_forms(engine, LOG_CEI, small.y_max, lb, ub, k_big=3)
    _check("plateau", LOG_CEI, res, small, lb, ub, small.y_max, tr, 3)
    assert res[0] == C.argbest(list(tr["key"]))[0] and np.isfinite(res[1])


# ---- 4. kind 6 alone, and a NaN candidate --------------------------------------------------------------------------------------------------
def test_kind_six_picks_the_largest_log_p_and_a_nan_candidate_wins(engine, small):
    lb, ub = CONFIGS["two-5-sigma"]
    small.resident(engine)
    tr = _truth(small, lb, ub, small.y_max)
    log_p = [-k for k in tr["key_feas"]]
    # acq_param and y_max are not read
    a = engine.acq_argbest(LOG_FEAS, XI, small.y_max, lb, ub, k_seeds=3, return_values=True)
    b = engine.acq_argbest(LOG_FEAS, 7.5, -1e30, lb, ub, k_seeds=3, return_values=True)
    assert a[0] == b[0] == max(range(small.M), key=lambda i: (log_p[i], -i))
    assert np.array_equal(R._bits(a[4]), R._bits(b[4])) and np.array_equal(a[2], b[2])
    Xn = small.Xc.copy()
    Xn[[1500, 700]] = np.nan
    post = small.resident(engine, fetch=True, Xc=Xn)
    assert np.isnan(post[1][0][700]) and np.isnan(post[0][0][1500])
    for kind in (LOG_CEI, LOG_FEAS):
        for k in (2, 5):
            bi, bv, si, sv, ys = engine.acq_argbest(kind, XI, small.y_max, lb, ub, k_seeds=k, return_values=True)
            assert bi == 700 and np.isnan(bv) and np.isnan(ys[[700, 1500]]).all() and np.isfinite(np.delete(ys, [700, 1500])).all()
            assert not np.isnan(sv).any()
            R._check_picks((bi, bv, si, sv, ys), k)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(engine, small):
    lb, ub = CONFIGS["two-contains"]
    small.resident(engine)
    before = engine.acq_argbest(LOG_CEI, XI, small.y_max, lb, ub, k_seeds=3, return_values=True)
    seeds = np.random.RandomState(1).uniform(size=(4, 2))
    box = np.array([[0.0, 1.0]] * 2)
    ym, ys = small.y_means, small.y_stds
    with pytest.raises(ValueError, match="GPBO_ACQ_LOG_FEAS needs at least one constraint"):
        engine.acq_argbest(LOG_FEAS, XI, small.y_max, k_seeds=3)
    with pytest.raises(ValueError, match="GPBO_ACQ_LOG_FEAS needs at least one constraint"):
        engine.polish_seeds(LOG_FEAS, XI, small.y_max, None, None, ym[:1], ys[:1], seeds, box)
    for kind, text in ((LOG_CEI, "GPBO_ACQ_LOG_CEI"), (LOG_FEAS, "GPBO_ACQ_LOG_FEAS")):
        with pytest.raises(ValueError, match=text):
            engine.evolve_mixed(kind, XI, small.y_max, ym[0], ys[0], [(0, 0, 1), (1, 1, 1)], np.array([[0.0, 1.0], [0.0, 5.0]]),
                                np.random.RandomState(2).uniform(size=(30, 2)), np.random.RandomState(3))
    for call in (lambda: engine.acq_argbest(4, XI, small.y_max, lb, ub, k_seeds=3),
                 lambda: engine.polish_seeds(4, XI, small.y_max, lb, ub, ym[:2], ys[:2], seeds, box),
                 lambda: engine.acq_argbest(7, XI, small.y_max, lb, ub, k_seeds=3)):
        with pytest.raises(ValueError, match="unknown acquisition"):
            call()
    with pytest.raises(ValueError, match="GPBO_ACQ_LOG_EI takes no constraints"):
        engine.acq_argbest(LOG_EI, XI, small.y_max, lb, ub, k_seeds=3)
    with pytest.raises(ValueError, match="GPBO_ACQ_LOG_EI takes no constraints"):
        engine.polish_seeds(LOG_EI, XI, small.y_max, lb, ub, ym[:2], ys[:2], seeds, box)
    small.resident(engine)                                  # after the refused calls a valid call answers as before them
    after = engine.acq_argbest(LOG_CEI, XI, small.y_max, lb, ub, k_seeds=3, return_values=True)
    assert before[0] == after[0] and np.array_equal(before[2], after[2]) and np.array_equal(R._bits(before[4]), R._bits(after[4]))


# ---- 6. the group form -------------------------------------------------------------------------------------------------------------------------
def test_a_one_device_group_gives_the_single_context_answer(engine, small):
    lb, ub = CONFIGS["two-constraints"]
    small.resident(engine)
    with GroupEngine([0]) as grp:
        small.resident(grp)
        for kind in (LOG_CEI, LOG_FEAS):
            one = engine.acq_argbest(kind, XI, small.y_max, lb, ub, k_seeds=6, return_values=True)
            many = grp.acq_argbest(kind, XI, small.y_max, lb, ub, k_seeds=6, return_values=True)
            assert one[0] == many[0] and R._bits([one[1]])[0] == R._bits([many[1]])[0]
            assert np.array_equal(one[2], many[2]) and np.array_equal(R._bits(one[3]), R._bits(many[3]))
            assert np.array_equal(R._bits(one[4]), R._bits(many[4]))


# ---- 7. the local search's objective and gradient ----------------------------------------------------------------------------------------------
def _objective(eng, kind, y_max, lb, ub, y_means, y_stds, pts):
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    n, d = pts.shape
    lb, ub = np.ascontiguousarray(lb, dtype=np.float64), np.ascontiguousarray(ub, dtype=np.float64)
    ym, ys = np.ascontiguousarray(y_means, dtype=np.float64), np.ascontiguousarray(y_stds, dtype=np.float64)
    f, g = np.empty(n), np.empty((n, d))
    eng._check(eng._lib.gpbo_debug_polish_objective(eng._h, int(kind), float(XI), float(y_max), int(lb.shape[0]), _lib.dptr(lb),
                                                    _lib.dptr(ub), _lib.dptr(ym), _lib.dptr(ys), _lib.dptr(pts), n, d, _lib.dptr(f),
                                                    _lib.dptr(g)))
    return f, g


GRADIENT_CASES = [(LOG_CEI, "two-contains"), (LOG_CEI, "two-30-sigma"), (LOG_CEI, "two-constraints"), (LOG_CEI, "ub-30-sigma"),
                  (LOG_FEAS, "lb-30-sigma"), (LOG_FEAS, "two-narrow-in-a-tail"), (LOG_FEAS, "two-constraints-far")]


@pytest.mark.parametrize("kind,name", GRADIENT_CASES)
def test_objective_and_gradient_of_the_lockstep_rounds(debug_engine, kind, name):
    """40 points: 32 in the square, 8 beside training points (small deviations: the band 30 sigma away is hundreds of sigma away there,
    where phi / p would be 0 / 0)"""
    eng = debug_engine
    case = _Case(eng, 64)
    lb, ub = CONFIGS[name]
    n_c = len(lb)
    pts = np.vstack([np.random.RandomState(6).uniform(size=(32, 2)), np.clip(case.X[:8] + 10.0 ** np.linspace(-4, -2, 8)[:, None], 0, 1)])
    f, g = _objective(eng, kind, case.y_max, lb, ub, case.y_means[:1 + n_c], case.y_stds[:1 + n_c], pts)
    posts = [eng.predict_grad(pts, slot=j, y_mean=case.y_means[j], y_std=case.y_stds[j]) for j in range(1 + n_c)]
    cons = [(float(lb[j]), float(ub[j]), posts[j + 1][0], posts[j + 1][1]) for j in range(n_c)]
    dcons = [(posts[j + 1][2], posts[j + 1][3]) for j in range(n_c)]
    tr = C.log_cei_truth(kind, posts[0][0], posts[0][1], case.y_max, XI, cons, posts[0][2], posts[0][3], dcons)
    assert tr["ok"].all()
    ref_f, ref_g = C.reference_values(kind, posts[0][0], posts[0][1], case.y_max, XI, cons, posts[0][2], posts[0][3], dcons)
    c_ref_f = T.worst(T.constants(ref_f, tr["key"], tr["w"], floor=0.0))
    c_ref_g = T.worst(C.constants(ref_g, tr["g"], tr["w_g"], tr["floor_g"]))
    c_f = T.worst(T.constants(f, tr["key"], tr["w"], floor=0.0))
    c_g = T.worst(C.constants(g, tr["g"], tr["w_g"], tr["floor_g"]))
    far = max(float(np.max(np.abs(np.where(np.isfinite(x), x, 0.0)))) for ab in tr["ab"] for x in ab)
    print(f"objective kind {kind} {name}: f c_dev {c_f:.3f} c_ref {c_ref_f:.3f}; g c_dev {c_g:.3f} c_ref {c_ref_g:.3f}; bounds up to {far:.0f} sigma away")
    assert np.isfinite(f).all() and np.isfinite(g).all()
    assert c_f <= 8.0 * max(c_ref_f, 1.0) and c_g <= 8.0 * max(c_ref_g, 1.0)
    if "30-sigma" in name:
        assert far >= 30.0
        product = C.reference_product(posts[0][0], posts[0][1], case.y_max, XI, cons)
        assert np.mean(product == 0.0) >= 0.5                # the product form has neither a value nor a slope there
    if kind == LOG_FEAS:                                     # slot 0's posterior, y_max and xi are not looked at
        eng.fit(case.X, case.norm[1][0], O.MATERN25, 0.2, C.SMALL_NOISE, slot=0)
        f2, g2 = _objective(eng, kind, 1e30, lb, ub, case.y_means[:1 + n_c], case.y_stds[:1 + n_c], pts)
        assert np.array_equal(R._bits(f), R._bits(f2)) and np.array_equal(R._bits(g), R._bits(g2))


def test_debug_polish_eval_takes_kind_five_as_log_ei_and_refuses_kind_six(debug_engine):
    import test_gpu_polish_fused as P

    eng = debug_engine
    case = _Case(eng, 64)
    pts = np.random.RandomState(6).uniform(size=(16, 2))
    a = P._polish_eval(eng, LOG_EI, XI, case.y_max, case.y_means[0], case.y_stds[0], pts)
    b = P._polish_eval(eng, LOG_CEI, XI, case.y_max, case.y_means[0], case.y_stds[0], pts)
    assert all(np.array_equal(R._bits(a[k]), R._bits(b[k])) for k in a)
    with pytest.raises(ValueError, match="GPBO_ACQ_LOG_FEAS"):
        P._polish_eval(eng, LOG_FEAS, XI, case.y_max, case.y_means[0], case.y_stds[0], pts)


# ---- 8. the local search -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", [(LOG_CEI, "two-5-sigma"), (LOG_CEI, "lb-contains"), (LOG_FEAS, "two-5-sigma")])
def test_local_searches_from_the_eight_best_candidates(debug_engine, kind, name):
    eng = debug_engine
    case = _Case(eng, C.SMALL_M)
    lb, ub = CONFIGS[name]
    ym, ys = case.y_means[:2], case.y_stds[:2]
    bi, bv, si, sv, _ = eng.acq_argbest(kind, XI, case.y_max, lb, ub, k_seeds=8)
    seeds = case.Xc[si]
    box = np.array([[0.0, 1.0]] * 2)
    f_seed, _ = _objective(eng, kind, case.y_max, lb, ub, ym, ys, seeds)
    x, f, status, rounds = eng.polish_seeds(kind, XI, case.y_max, lb, ub, ym, ys, seeds, box)
    print(f"polish kind {kind} {name}: status {status.tolist()} rounds {rounds} f_seed [{f_seed.min():.4f}, {f_seed.max():.4f}] "
          f"f [{f.min():.4f}, {f.max():.4f}] best candidate {bv:.4f}")
    assert np.all(status < 2)                                # 0 / 1: converged
    assert np.all(x >= 0.0) and np.all(x <= 1.0)
    assert np.all(np.isfinite(f)) and np.all(f <= f_seed)    # the first evaluation of a run is its seed's, by the same code
    best = int(np.argmin(f))
    posts = [eng.predict(x[best:best + 1], slot=j, y_mean=ym[j], y_std=ys[j]) for j in range(2)]
    cons = [(float(lb[0]), float(ub[0]), posts[1][0], posts[1][1])]
    f_ref = C.reference_values(kind, posts[0][0], posts[0][1], case.y_max, XI, cons)[0]
    tr = C.log_cei_truth(kind, posts[0][0], posts[0][1], case.y_max, XI, cons)
    slack = 2.0 * 8.0 * T.EPS * float(tr["w"][0])            # the restatement's and the device's rounding at that point, c <= 8 each
    assert f_ref <= bv + slack


# ---- 9. the seam -----------------------------------------------------------------------------------------------------------------------------------
D, M = 3, 2000
BOUNDS = np.array([[0.0, 1.0]] * D)
SEAM_LB, SEAM_UB = np.array([-0.2]), np.array([0.35])
RECORDED = {"fit": "fit", "fit_append": "fit", "set_candidates": "candidates", "generate_candidates_like": "candidates",
            "generate_candidates": "candidates", "generate_candidates_mixed": "candidates", "acq_argbest": "acq_argbest",
            "polish_seeds": "polish_seeds", "evolve_mixed": "evolve_mixed"}


def _seam_driver(engine, feasible):
    X = np.random.RandomState(140).uniform(size=(40, D))
    y = np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1]) + X[:, 2] ** 2
    cv = np.cos(2.0 * X.sum(1)) + (0.0 if feasible else 2.0)
    drv = B.Driver(engine, X, y, BOUNDS, A.LogConstrainedExpectedImprovement(), seed=7, n_random=M)
    cm = HipConstraintModel(None, SEAM_LB, SEAM_UB, engine=engine, random_state=np.random.RandomState(3))
    drv._space = FloatSpace({f"x{j}": tuple(b) for j, b in enumerate(BOUNDS)}, constraint=cm)
    drv._space.register_bulk(X, y, cv)
    return drv, y, cv


@pytest.mark.parametrize("feasible", [True, False], ids=["a-feasible-observation", "no-feasible-observation"])
def test_one_suggest_on_the_engine(engine, monkeypatch, feasible):
    drv, y, cv = _seam_driver(engine, feasible)
    calls = []
    for name, label in RECORDED.items():
        real = getattr(engine, name)

        def recorder(*args, _real=real, _label=label, **kw):
            calls.append((_label, args[0]) if _label in ("acq_argbest", "polish_seeds") else (_label,))
            return _real(*args, **kw)

        monkeypatch.setattr(engine, name, recorder)
    policy = drv._acquisition_function
    x = policy.suggest(gp=drv._gp, target_space=drv._space, n_random=M, n_smart=10, fit_gp=True, random_state=drv._random_state)
    kind = LOG_CEI if feasible else LOG_FEAS
    print(f"seam ({'feasible' if feasible else 'infeasible'}): calls {calls}, x {x}")
    assert calls == [("fit",), ("fit",), ("candidates",), ("acq_argbest", kind), ("polish_seeds", kind)]
    assert np.all(x >= BOUNDS[:, 0]) and np.all(x <= BOUNDS[:, 1]) and np.isfinite(x).all()
    ok = (cv >= SEAM_LB[0]) & (cv <= SEAM_UB[0])
    assert ok.any() == feasible
    assert policy.y_max == (float(y[ok].max()) if feasible else None)
    # the suggestion's objective is finite, and no worse than what the random stage alone returns from the same stream
    policy._acq_kind = kind
    try:
        f = policy._get_acq(gp=drv._gp, constraint=drv._space.constraint)
        assert np.isfinite(f(x)).all()
    finally:
        policy._acq_kind = LOG_CEI
