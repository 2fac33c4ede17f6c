"""GPU (-m gpu): gpmo_cnhvi_greedy, greedy noisy EHVI under noisy constraints (include/gpmo.h), and suggest_constrained_qnehvi /
ParetoOptimizer(constraints=...) end to end.

Cases: the two models of tests/test_gpu_ehvi.py — (N = 40, d = 3, Matern 2.5) and (N = 300, d = 17, RBF) — over M = 1000 and 257
(both thread rules of qnei_items), T = 1, 10, 48 and 256 draws, C = 1 and 2, F = 64, q = 6, n_base = N + 3 pending; one case at
M = 2^17, T = 16 for the wide evaluation workgroup.  Everything is checked BIT FOR BIT:

  * the raw draws in values_out against gpbo_sample_paths per slot and group; viol_out against gpbo_sample_paths_constrained's for
    C = 1 (the constraint's model moved to slot 1 for that call) and against cmo_truth's fold for C = 2;
  * the fronts before and after, every step's keys, the picks, gains and pick_feasible against cmo_truth's replay ON THE FETCHED RAW
    VALUES — the draws are gpbo_sample_paths' own, so the truth's input is what an existing, separately tested call made;
  * with every bound infinite: picks, gains, keys and fronts are gpbo_qnhvi_greedy's.
The bounds are quantiles of the fetched constraint draws and ref is the lowest quantile pair of the fetched base values at which
the TRUTH (cmo_truth.rule alone) meets the conditions of a non-trivial case: the share of feasible (draw, candidate) pairs in
[0.2, 0.8], a draw that starts with an empty front and one with at least 3 points, a pick that differs from the unconstrained
batch's, a pick_feasible strictly between 0 and 1.  Every case with T >= 10 asserts all of them (SEARCH says where the two T = 10
cases find theirs)."""
import functools

import numpy as np
import pytest

import cmo_truth as CM
import cnei_truth as CT
import matern_family_truth as F
import qnehvi_truth as QT
from bayesianoptimization_amd import _lib
from bayesianoptimization_amd.cqnehvi import suggest_constrained_qnehvi
from bayesianoptimization_amd.engine import GpEngine, GroupEngine
from bayesianoptimization_amd.multiobjective import ParetoOptimizer

pytestmark = pytest.mark.gpu

INF = np.inf
Q = 6
MODELS = {"n40": (40, 3, F.MATERN25), "n300": (300, 17, F.RBF)}
#: name -> (model, M, G, S, C, conditions asserted)
CASES = {
    "n40-m1000-t10-c1": ("n40", 1000, 2, 5, 1, True),
    "n40-m257-t48-c2": ("n40", 257, 3, 16, 2, True),
    "n300-m257-t10-c2": ("n300", 257, 2, 5, 2, True),
    "n300-m1000-t48-c1": ("n300", 1000, 3, 16, 1, True),
    "n40-m257-t1-c1": ("n40", 257, 1, 1, 1, False),
    "n40-m1000-t256-c1": ("n40", 1000, 16, 16, 1, True),
    "n40-m131072-t16-c1": ("n40", 1 << 17, 1, 16, 1, False),
}
#: where `bounds_and_ref` looks first for the two T = 10 cases — (bands, objective 0's ref quantiles, objective 1's).  Ten draws all
#: see nearly the same values at the observed points, so the fronts differ between draws only through the base points near an edge
#: of the band: a band off the centre (a quarter of the constraint's draws) and a reference point near the lower end of the base
#: values (n40) or above their median (n300) leave one draw without a front and others with three points and more.  Found on the
#: NumPy path truth; the test asserts the conditions on what the device drew.
SEARCH = {
    "n40-m1000-t10-c1": (((0.0, 0.25),), (0.0, 0.1), (0.28, 0.14, 0.16, 0.2)),
    "n300-m257-t10-c2": (((0.1, 0.35),), (0.6, 0.64), (0.76, 0.78, 0.8)),
}


@functools.lru_cache(maxsize=None)
def case_of(name):
    model, M, G, S, C, _ = CASES[name]
    N, d, kind = MODELS[model]
    return CT.Case(C=C + 1, Ns=N, M=M, Fn=64, d=d, G=G, S=S, B=N + 3, kinds=[kind] * (C + 2), per_dim=True, seed=len(name))


def run(eng, c, lb, ub, ref, q=Q, **kw):
    kw.setdefault("return_values", True)
    kw.setdefault("return_keys", True)
    kw.setdefault("return_fronts", True)
    return eng.cnehvi_greedy(c.draws, q, lb, ub, ref, base=c.base, y_mean=c.y_mean, y_std=c.y_std, **kw)


def probe(eng, c):
    """the raw draws (values, base_values) by a first call with free bounds"""
    free = np.full(c.C - 1, INF)
    out = run(eng, c, -free, free, np.array([-1e300, -1e300]), q=1, return_keys=False, return_fronts=False)
    return out["values"], out["base_values"]


#: the default search of `bounds_and_ref`, in this order: the constraints' band as quantiles of their draws (0: no lower bound, 1: no
#: upper bound), ref as quantiles of the base values
BANDS = ((0.2, 0.8), (0.3, 0.7), (0.35, 0.65), (0.1, 0.9), (0.4, 0.6))
REF_QUANTILES = (0.3, 0.5, 0.1, 0.7, 0.0, 0.8, 0.9)


def bounds_and_ref(c, values, base_values, conditions, search=None):
    """The bounds from quantiles of the constraints' draws (with two constraints the second is one-sided); ref from quantiles of the
    base values per objective.  With `conditions` the first combination of `search` (default BANDS x REF_QUANTILES^2) at which the
    TRUTH meets the conditions on the masked fronts and on the feasible share — a draw without a front, a draw with at least three
    points, the share of feasible (draw, candidate) pairs in [0.2, 0.8]; without, the first of each."""
    n_c = c.C - 1
    bands, ref0, ref1 = (BANDS, REF_QUANTILES, REF_QUANTILES) if search is None else search
    for lo, hi in bands:
        lb = np.array([np.quantile(values[2 + j], lo) if lo > 0 else -INF for j in range(n_c)])
        ub = np.array([np.quantile(values[2 + j], hi) if hi < 1 else INF for j in range(n_c)])
        if n_c == 2:
            ub[1] = INF                                    # a one-sided constraint
        if not conditions:
            return lb, ub, np.array([np.quantile(base_values[0], 0.5), np.quantile(base_values[1], 0.5)])
        share = float(np.mean(CM.violations(values, lb, ub, c.y_std) == 0.0))
        if not 0.2 <= share <= 0.8:
            continue
        gb = CM.masked_draws(base_values, lb, ub, c.y_std)[0]
        for r0 in ref0:
            for r1 in ref1:
                ref = np.array([np.quantile(base_values[0], r0), np.quantile(base_values[1], r1)]) - 1e-9
                sizes = np.array([f.shape[0] for f in QT.fronts_of(gb, ref)])
                if (sizes == 0).any() and (sizes >= 3).any():
                    return lb, ub, ref
    raise AssertionError(f"{c.what}: no band and reference point leave one draw without a front and one with three points")


def check_fronts(out, before, after):
    for block, want in ((0, before), (1, after)):
        got = QT.unpack(out["front_size"][block], out["fronts"][block])
        assert QT.same_fronts(got, want), f"fronts block {block}"


@pytest.mark.parametrize("name", list(CASES))
def test_the_whole_call_bit_for_bit(engine, name):
    c = case_of(name)
    conditions = CASES[name][5]
    n_c, T, M = c.C - 1, c.T, c.M
    c.fit(engine)
    values, base_values = probe(engine, c)
    assert np.isfinite(values).all() and np.isfinite(base_values).all()
    # the raw draws are gpbo_sample_paths', per slot and group
    for j in range(2 + n_c):
        for g, (om, ph, w, eps) in enumerate(c.draws[j]):
            if T > 48 and g not in (0, c.G - 1):
                continue                                # (T = 256: the first and the last group of every slot)
            rows = engine.sample_paths(om, ph, w, eps, slot=j, y_mean=c.y_mean[j], y_std=c.y_std[j], return_values=True)[2]
            assert rows.tobytes() == values[j, g * c.S:(g + 1) * c.S].tobytes(), (j, g)
    lb, ub, ref = bounds_and_ref(c, values, base_values, conditions, SEARCH.get(name))
    truth = CM.rule(values, base_values, lb, ub, c.y_std, ref, Q)
    if conditions:      # on the truth alone: the fronts' variety, in one call
        sizes = np.array([f.shape[0] for f in truth["fronts_before"]])
        assert (sizes == 0).any() and (sizes >= 3).any(), sizes
    out = run(engine, c, lb, ub, ref)
    assert out["values"].tobytes() == values.tobytes() and out["base_values"].tobytes() == base_values.tobytes()
    assert out["viol"].tobytes() == truth["viol"].tobytes()
    assert out["keys"].tobytes() == truth["keys"].tobytes()
    assert np.array_equal(out["index"], truth["index"])
    assert out["gain"].tobytes() == truth["gain"].tobytes() and out["feasible"].tobytes() == truth["feasible"].tobytes()
    check_fronts(out, truth["fronts_before"], truth["fronts_after"])
    # the optional outputs change nothing
    lean = run(engine, c, lb, ub, ref, return_values=False, return_keys=False, return_fronts=False)
    assert np.array_equal(lean["index"], out["index"]) and lean["gain"].tobytes() == out["gain"].tobytes()
    assert lean["feasible"].tobytes() == out["feasible"].tobytes()
    # every bound infinite: gpbo_qnhvi_greedy's answer
    free = np.full(n_c, INF)
    plain = engine.qnehvi_greedy(c.draws[:2], Q, ref, base=c.base, y_mean=c.y_mean[:2], y_std=c.y_std[:2], return_keys=True,
                                 return_fronts=True)
    unmasked = run(engine, c, -free, free, ref)
    assert np.array_equal(unmasked["index"], plain["index"]) and unmasked["gain"].tobytes() == plain["gain"].tobytes()
    assert unmasked["keys"].tobytes() == plain["keys"].tobytes() and (unmasked["feasible"] == 1.0).all()
    for block in (0, 1):
        assert QT.same_fronts(QT.unpack(unmasked["front_size"][block], unmasked["fronts"][block]),
                              QT.unpack(plain["front_size"][block], plain["fronts"][block]))
    if conditions:      # on the truth alone
        share = float(np.mean(truth["viol"] == 0.0))
        assert 0.2 <= share <= 0.8, share
        assert not np.array_equal(truth["index"], plain["index"]), "the constraints move no pick"
        assert ((truth["feasible"] > 0) & (truth["feasible"] < 1)).any()
        # each slip changes an output.  Masking objective 1 instead of 0 cannot change a key or a front — a strip's area is 0 and an
        # insertion fails with EITHER coordinate at -inf —; what it changes is pick_feasible, which counts objective 0's -inf
        wrong = CM.rule(values, base_values, lb, ub, c.y_std, ref, Q, mask_objective=1)
        assert wrong["keys"].tobytes() == truth["keys"].tobytes() and wrong["feasible"].tobytes() != truth["feasible"].tobytes()
        if n_c == 2:      # the constraints' y_std swapped: viol_out's bits (the mask, which asks viol == 0, cannot see it)
            assert CM.violations(values, lb, ub, c.y_std, swap=True).tobytes() != truth["viol"].tobytes()
        unmasked_base = CM.rule(values, base_values, lb, ub, c.y_std, ref, Q, mask_base=False)
        assert not np.array_equal(unmasked_base["index"], truth["index"]) or unmasked_base["keys"].tobytes() != truth["keys"].tobytes()


def test_viol_out_is_the_constrained_samplers_for_one_constraint(engine):
    c = case_of("n40-m1000-t10-c1")
    c.fit(engine)
    values, base_values = probe(engine, c)
    lb, ub, ref = bounds_and_ref(c, values, base_values, False)
    viol = run(engine, c, lb, ub, ref)["viol"]
    s = c.slots[2]
    engine.fit(s["X"], s["yn"], s["kind"], s["ls"], CT.NOISE, slot=1)      # the constraint's model into the sampler's slot
    for g in range(c.G):
        got = engine.sample_paths_constrained([c.draws[0][g], c.draws[2][g]], lb, ub, c.y_mean[[0, 2]], c.y_std[[0, 2]],
                                              return_values=True)[5]
        assert got.tobytes() == viol[g * c.S:(g + 1) * c.S].tobytes(), g


def test_nan_candidates(engine):
    c = case_of("n40-m257-t48-c2")
    Xc = np.array(c.Xc)
    Xc[[200, 13]] = np.nan
    c.fit(engine, Xc)
    values, base_values = probe(engine, c)
    assert np.isnan(values[:, :, [13, 200]]).all()
    lb, ub, ref = bounds_and_ref(c, np.delete(values, [13, 200], axis=2), base_values, False)
    out = run(engine, c, lb, ub, ref)
    truth = CM.rule(values, base_values, lb, ub, c.y_std, ref, Q)
    assert list(out["index"][:2]) == [13, 200] and np.isnan(out["gain"][:2]).all() and np.isnan(out["feasible"][:2]).all()
    assert np.array_equal(out["index"], truth["index"]) and out["keys"].tobytes() == truth["keys"].tobytes()
    assert out["feasible"].tobytes() == truth["feasible"].tobytes()
    check_fronts(out, truth["fronts_before"], truth["fronts_after"])
    assert QT.same_fronts(truth["fronts_before"], QT.greedy(truth["masked"], truth["fronts_before"], ref, 2)[3]), "a NaN pick moves a front"


def test_reader_only(engine):
    c = case_of("n40-m1000-t10-c1")
    c.fit(engine)
    values, base_values = probe(engine, c)
    lb, ub, ref = bounds_and_ref(c, values, base_values, False)
    for j in range(3):
        engine.posterior(j, c.y_mean[j], c.y_std[j], fetch=False)
    before = engine.acq_argbest(0, 2.0, k_seeds=4, return_values=True)
    alpha = [engine.get_alpha(40, j) for j in range(3)]
    rows = engine.get_candidate_rows(np.arange(c.M), c.d)
    run(engine, c, lb, ub, ref)
    after = engine.acq_argbest(0, 2.0, k_seeds=4, return_values=True)
    for a, b in zip(before, after):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    assert all(np.array_equal(a, engine.get_alpha(40, j)) for j, a in enumerate(alpha))
    assert np.array_equal(rows, engine.get_candidate_rows(np.arange(c.M), c.d))


@functools.lru_cache(maxsize=None)
def small_case():
    """two objectives and one constraint over M = 63 candidates (q = 64 exceeds them), 2 x 5 draws, 43 base points"""
    return CT.Case(C=2, Ns=40, M=63, Fn=64, d=3, G=2, S=5, B=43, kinds=[F.MATERN25] * 3, per_dim=True, seed=1)


def test_refusals_at_the_library_and_a_valid_call_behind_them():
    """Every refusal include/gpmo.h lists, asked at the C boundary (the engine's own checks never see these calls), on a context of
    its own — which slots were ever fitted is part of what is refused —, then the valid call answers as before."""
    from bayesianoptimization_amd._lib import dptr, iptr

    c = small_case()
    with GpEngine(0) as eng:
        c.fit(eng)
        G, S, Fn, d, C = c.G, c.S, c.F, c.d, 1
        flat = [t for groups in c.draws for t in groups]
        omega = np.ascontiguousarray(np.concatenate([t[0].ravel() for t in flat]))
        phase = np.ascontiguousarray(np.concatenate([t[1] for t in flat]))
        w = np.ascontiguousarray(np.concatenate([t[2].ravel() for t in flat]))
        eps = np.ascontiguousarray(np.concatenate([t[3].ravel() for t in flat]))
        base = np.ascontiguousarray(c.base)
        y_mean, y_std = np.ascontiguousarray(c.y_mean), np.ascontiguousarray(c.y_std)
        values, base_values = probe(eng, c)
        lb, ub, ref = (np.ascontiguousarray(v) for v in bounds_and_ref(c, values, base_values, False))
        pi, pg, pf = np.empty(64, dtype=np.int64), np.empty(64), np.empty(64)

        def call(h=None, n_constraints=C, ym=y_mean, ys=y_std, lo=lb, hi=ub, n_groups=G, n_paths=S, n_features=Fn, draws=None,
                 rf=ref, bp=dptr(base), n_base=c.B, dd=d, q=4, outs=None, frames=None):
            draws = [dptr(omega), dptr(phase), dptr(w), dptr(eps)] if draws is None else draws
            outs = [iptr(pi), dptr(pg), dptr(pf)] if outs is None else outs
            frames = [dptr(ym), dptr(ys), dptr(lo), dptr(hi)] if frames is None else frames
            return eng._lib.gpmo_cnhvi_greedy(eng._h if h is None else h, n_constraints, *frames, n_groups, n_paths, n_features, *draws,
                                              None if rf is None else dptr(rf), bp, n_base, dd, q, 0, *outs, None, None, None, None, None,
                                              None)

        want = run(eng, c, lb, ub, ref, q=4)
        assert call() == _lib.GPBO_OK and np.array_equal(pi[:4], want["index"]) and pg[:4].tobytes() == want["gain"].tobytes()
        # n_constraints outside [1, GPBO_MAX_MODELS - 2] (7 would overrun the slots' table); the counts outside their ranges
        for bad in (0, -1, 7, 8, 100):
            assert call(n_constraints=bad) == _lib.ERR_INVALID, bad
        assert call(n_groups=0) == _lib.ERR_INVALID and call(n_groups=17) == _lib.ERR_INVALID
        assert call(n_paths=0) == _lib.ERR_INVALID and call(n_paths=17) == _lib.ERR_INVALID
        assert call(n_features=0) == _lib.ERR_INVALID and call(n_features=4097) == _lib.ERR_INVALID
        # a NULL among y_mean / y_std / lb / ub, the draw inputs, ref, pick_idx / pick_gain / pick_feasible
        for k in range(4):
            a = [dptr(y_mean), dptr(y_std), dptr(lb), dptr(ub)]
            a[k] = None
            assert call(frames=a) == _lib.ERR_INVALID
            a = [dptr(omega), dptr(phase), dptr(w), dptr(eps)]
            a[k] = None
            assert call(draws=a) == _lib.ERR_INVALID
        for k in range(3):
            a = [iptr(pi), dptr(pg), dptr(pf)]
            a[k] = None
            assert call(outs=a) == _lib.ERR_INVALID
        assert call(rf=None) == _lib.ERR_INVALID
        # a y_std not finite or not positive, a y_mean not finite, in any slot
        for j in range(2 + C):
            for bad in (0.0, -1.0, np.inf, np.nan):
                v = y_std.copy()
                v[j] = bad
                assert call(ys=v) == _lib.ERR_INVALID
            for bad in (np.inf, np.nan):
                v = y_mean.copy()
                v[j] = bad
                assert call(ym=v) == _lib.ERR_INVALID
        # a NaN bound, lb >= ub; infinite sides are allowed; a ref not finite
        assert call(lo=np.array([np.nan])) == _lib.ERR_INVALID and call(hi=np.array([np.nan])) == _lib.ERR_INVALID
        assert call(lo=ub.copy(), hi=ub.copy()) == _lib.ERR_INVALID and call(lo=ub.copy(), hi=lb.copy()) == _lib.ERR_INVALID
        assert call(lo=np.array([-INF]), hi=np.array([INF])) == _lib.GPBO_OK
        for bad in (np.nan, np.inf, -np.inf):
            for k in range(2):
                v = ref.copy()
                v[k] = bad
                assert call(rf=v) == _lib.ERR_INVALID
        # n_base outside [0, GPBO_MAX_QNEHVI_BASE], n_base > 0 with a NULL or non-finite base, d not the slots'
        assert call(n_base=-1) == _lib.ERR_INVALID and call(n_base=16385) == _lib.ERR_INVALID
        assert call(bp=None, n_base=1) == _lib.ERR_INVALID and call(bp=None, n_base=0) == _lib.GPBO_OK
        for bad in (np.nan, np.inf):
            bb = base.copy()
            bb[3, 1] = bad
            assert call(bp=dptr(bb)) == _lib.ERR_INVALID
        assert call(dd=d + 1) == _lib.ERR_INVALID and call(dd=d + 1, bp=None, n_base=0) == _lib.ERR_INVALID
        # q outside [1, GPBO_MAX_SEEDS], or q > M
        assert call(q=0) == _lib.ERR_INVALID and call(q=65) == _lib.ERR_INVALID
        assert call(q=63) == _lib.GPBO_OK and call(q=64) == _lib.ERR_INVALID             # M = 63
        assert call(ctypes_null()) == _lib.ERR_INVALID                                   # a NULL context
        # the engine's own refusals, as exceptions
        with pytest.raises(ValueError, match="2 \\+ C lists"):
            eng.cnehvi_greedy(c.draws[:2], 2, lb, ub, ref)
        with pytest.raises(ValueError, match="n_groups"):
            eng.cnehvi_greedy([g * 9 for g in c.draws], 2, lb, ub, ref)
        with pytest.raises(ValueError, match="same non-empty list"):
            eng.cnehvi_greedy([c.draws[0], c.draws[1], c.draws[2][:1]], 2, lb, ub, ref)
        with pytest.raises(ValueError, match="lb / ub"):
            eng.cnehvi_greedy(c.draws, 2, [0.0, 1.0], [1.0, 2.0], ref)
        with pytest.raises(ValueError, match="ref must hold"):
            eng.cnehvi_greedy(c.draws, 2, lb, ub, [0.0, 0.0, 0.0])
        with pytest.raises(ValueError, match="base"):
            eng.cnehvi_greedy(c.draws, 2, lb, ub, ref, base=np.zeros((1, d + 1)))
        with pytest.raises(ValueError, match="q out of range"):
            run(eng, c, lb, ub, ref, q=65)
        # GPBO_ERR_STATE: a slot that was never fitted (C = 2 reads slot 3), a constraint slot that gpbo_lml left unfitted
        two = [np.ascontiguousarray(np.concatenate([v, v[-1:]])) for v in (y_mean, y_std)]
        big = [np.ascontiguousarray(np.concatenate([v, v[len(v) * 2 // 3:]])) for v in (omega, phase, w, eps)]
        assert call(n_constraints=2, ym=two[0], ys=two[1], lo=np.tile(lb, 2), hi=np.tile(ub, 2), draws=[dptr(v) for v in big]) == _lib.ERR_STATE
        s = c.slots[2]
        eng.lml(s["X"], s["yn"], s["kind"], s["ls"], CT.NOISE, slot=2)
        with pytest.raises(_lib.GpboError, match="not been fitted"):
            run(eng, c, lb, ub, ref, q=2)
        assert call() == _lib.ERR_STATE
        c.fit(eng)
        # ... a fit pending on a slot (the engine would wait for it: asked at the C boundary)
        with eng.overlapped_fits():
            eng.fit(s["X"], s["yn"], s["kind"], s["ls"], CT.NOISE, slot=2)
            assert call() == _lib.ERR_STATE
        assert call() == _lib.GPBO_OK
        # ... candidates of another d
        eng.set_candidates(np.random.RandomState(1).uniform(size=(10, d + 1)))
        with pytest.raises(_lib.GpboError, match="dimension"):
            run(eng, c, lb, ub, ref, q=2)
        # ... no resident candidates: a context that never had any
        with GpEngine(0) as fresh:
            assert call(h=fresh._h) == _lib.ERR_STATE
            for j, sl in enumerate(c.slots):
                fresh.fit(sl["X"], sl["yn"], sl["kind"], sl["ls"], CT.NOISE, slot=j)
            with pytest.raises(_lib.GpboError, match="no candidates"):
                run(fresh, c, lb, ub, ref, q=2)
        # a device group
        with pytest.raises(NotImplementedError, match="device group"):
            GroupEngine.cnehvi_greedy(object.__new__(GroupEngine), c.draws, 2, lb, ub, ref)
        # behind all of them the valid call answers as before
        eng.set_candidates(c.Xc)
        got = run(eng, c, lb, ub, ref, q=4)
        for k in ("index", "gain", "feasible", "keys", "viol"):
            assert got[k].tobytes() == want[k].tobytes(), k


def ctypes_null():
    import ctypes

    return ctypes.c_void_p(None)


def _toy(X):
    s = X.sum(axis=1)
    return np.column_stack([np.sin(3.0 * s) + X[:, 0], np.cos(2.0 * s) + X[:, 1]]), X[:, 0] - X[:, 1] + 0.3 * np.sin(4.0 * s)


def _pareto(engine, n=30, seed=11):
    rs = np.random.RandomState(seed)
    opt = ParetoOptimizer({"a": (0.0, 1.0), "b": (0.0, 1.0), "c": (0.0, 1.0)}, 2, [-1.5, -1.5], random_state=seed, engine=engine,
                          n_restarts_optimizer=1, constraints=[(-0.2, INF)])
    X = rs.uniform(size=(n, 3))
    Y, c = _toy(X)
    for x, y, v in zip(X, Y, c):
        opt.register(x, y, [v])
    return opt


def test_pareto_optimizer_with_constraints_and_the_batch_end_to_end(engine):
    opt = _pareto(engine)
    feas = opt.feasible
    assert 0 < feas.sum() < len(opt)
    params, targets = opt.front
    assert all(any(np.array_equal(p, row) for row in opt.params[feas]) for p in params)
    x, info = opt.suggest(n_random=2000, return_info=True)
    assert set(x) == {"a", "b", "c"} and all(0.0 <= v <= 1.0 for v in x.values())
    assert np.isfinite(info["value"]) and 0 <= info["index"] < 2000 and info["front_size"] == targets.shape[0]
    picks, binfo = suggest_constrained_qnehvi(opt, 4, n_random=2000, n_draws=20, n_features=128, pending=[x], return_info=True)
    assert len(picks) == 4 and len({tuple(p.values()) for p in picks}) == 4
    assert binfo["n_draws"] == 20 and binfo["gain"].shape == (4,) and (binfo["gain"][:1] > 0).all()
    assert ((binfo["feasible"] >= 0) & (binfo["feasible"] <= 1)).all()
    assert binfo["front_size_after"] >= 1
    with pytest.raises(ValueError, match="use suggest_qnehvi"):
        suggest_constrained_qnehvi(ParetoOptimizer({"a": (0.0, 1.0)}, 2, [0.0, 0.0], engine=engine), 2)
