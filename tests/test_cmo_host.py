"""CPU: the rules of include/gpmo.h in tests/cmo_truth.py, and ParetoOptimizer(constraints=...) / suggest_constrained_qnehvi over a
recording engine double.

  * the masked staircase: qnehvi_truth's HVI on g0 (objective 0 masked to -inf where the draw's constraints fail) equals the
    hypervolume a point adds to the front of the draw's FEASIBLE points, computed directly with multiobjective.hypervolume;
  * discrimination: each plausible slip — leaving the base unmasked, a constraint order swap with unequal y_std, s added in
    product form — changes a pick, a key or the violations' bits; masking objective 1 instead of 0 provably changes no key (a
    strip's area is 0 with either coordinate at -inf) and is caught by pick_feasible instead;
  * ParetoOptimizer with constraints and suggest_constrained_qnehvi: order of calls, RandomState consumption, feasible-only
    front, every refusal; constraints=None is call for call what it was."""
import contextlib

import numpy as np
import pytest

import batch_truth as B
import cmo_truth as CM
import ehvi_truth as ET
import qnehvi_truth as Q
import test_ehvi_host as EH
import test_qnehvi_host as QH
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd._suggest import draw_layout
from bayesianoptimization_amd.cqnehvi import suggest_constrained_qnehvi
from bayesianoptimization_amd.multiobjective import ParetoOptimizer, box_decomposition, hypervolume, pareto_front
from bayesianoptimization_amd.thompson import spectral_draw

INF = np.inf


# ---- the truths ---------------------------------------------------------------------------------------------------------------------
def test_the_masked_staircase_is_the_hypervolume_added_to_the_feasible_front():
    rs = np.random.RandomState(5)
    ref = np.array([0.0, 0.0])
    for trial in range(40):
        n_base, n_cand = int(rs.randint(0, 9)), 12
        base = np.round(rs.uniform(-0.2, 1.0, size=(3, 1, n_base)), 2)          # (2 + C, T = 1, B): ties on purpose
        cand = np.round(rs.uniform(-0.2, 1.2, size=(3, 1, n_cand)), 2)
        lb, ub, y_std = np.array([0.2]), np.array([0.9]), np.array([1.0, 1.0, 0.5])
        gb = CM.masked_draws(base, lb, ub, y_std)[0]
        g, viol = CM.masked_draws(cand, lb, ub, y_std)
        front = Q.fronts_of(gb, ref)[0]
        feasible_base = base[:2, 0][:, (base[2, 0] >= lb[0]) & (base[2, 0] <= ub[0])].T
        assert np.array_equal(front, Q.front_of(feasible_base, ref)), "the front is the feasible points' front"
        got = Q.hvi(g[0, 0], g[1, 0], front, ref)
        hv0 = hypervolume(feasible_base, ref)
        for i in range(n_cand):
            ok = viol[0, i] == 0.0
            want = hypervolume(np.vstack([feasible_base, cand[:2, 0, i][None]]), ref) - hv0 if ok else 0.0
            assert got[i] == pytest.approx(want, abs=1e-12), (trial, i)
            assert ok or (got[i] == 0.0 and not np.signbit(got[i])), "an infeasible candidate adds +0"
            assert (Q.insert(front, g[:, 0, i], ref) is front) or ok, "an infeasible pick leaves the front as it is"


def _synthetic(seed=0, T=6, M=40, B=9):
    rs = np.random.RandomState(seed)
    values = rs.uniform(0.0, 1.0, size=(4, T, M))
    base = rs.uniform(0.0, 0.8, size=(4, T, B))
    return values, base, np.array([0.25, 0.3]), np.array([0.85, INF]), np.array([1.0, 1.0, 0.3, 1.7]), np.array([0.1, 0.1])


def test_each_slip_changes_a_pick_or_a_key():
    values, base, lb, ub, y_std, ref = _synthetic()
    truth = CM.rule(values, base, lb, ub, y_std, ref, 5)
    share = np.mean(truth["viol"] == 0.0)
    assert 0.2 <= share <= 0.8 and ((truth["feasible"] > 0) & (truth["feasible"] < 1)).any()
    # masking objective 1 instead of 0 cannot change a key or a front (a strip's area is 0 and an insertion fails with EITHER
    # coordinate at -inf): the output it changes is pick_feasible, which counts objective 0's -inf
    wrong = CM.rule(values, base, lb, ub, y_std, ref, 5, mask_objective=1)
    assert wrong["keys"].tobytes() == truth["keys"].tobytes() and wrong["feasible"].tobytes() != truth["feasible"].tobytes()
    other = CM.rule(values, base, lb, ub, y_std, ref, 5, mask_base=False)
    assert not np.array_equal(other["index"], truth["index"]) or other["keys"].tobytes() != truth["keys"].tobytes()
    # the constraints' order with unequal y_std: a two-term sum commutes, so what a swap can get wrong is WHICH y_std divides
    # which term — that changes viol_out's bits wherever a term is not 0, and no key (the mask only asks viol == 0)
    swapped = CM.violations(values, lb, ub, y_std, swap=True)
    assert swapped.tobytes() != truth["viol"].tobytes() and np.array_equal(swapped == 0.0, truth["viol"] == 0.0)
    # s added in product form
    rs = np.random.RandomState(1)
    mu, sd = rs.uniform(0.0, 1.0, size=(3, 50)), rs.uniform(0.05, 0.3, size=(3, 50))
    front = ET.random_front(5, 2, 5, lo=0.3, hi=0.9)
    _n, levels, lo, hi = box_decomposition(front, np.zeros(2))
    rows = ET.trim(_n, levels)
    right = CM.cehvi_keys(mu, sd, rows, (lo, hi), [0.4], [INF], True)
    wrong = CM.cehvi_keys(mu, sd, rows, (lo, hi), [0.4], [INF], True, product_slip=True)
    assert int(np.argmin(right)) != int(np.argmin(wrong)) or right.tobytes() != wrong.tobytes()
    prod = CM.cehvi_keys(mu, sd, rows, (lo, hi), [0.4], [INF], False)
    fin = np.isfinite(right) & (prod < 0)
    assert np.allclose(np.log(-prod[fin]), -right[fin], rtol=1e-12), "the two forms are one quantity"
    free = CM.cehvi_keys(mu, sd, rows, (lo, hi), [-INF], [INF], False)
    assert free.tobytes() == (-ET.ehvi_values(mu[:2], sd[:2], rows, lo, hi)).tobytes()


# ---- ParetoOptimizer(constraints=...) over the engine double ------------------------------------------------------------------------
class EhviEngine(EH.EhviFakeEngine):
    def cehvi_argbest(self, levels, cell_lo, cell_hi, lb, ub, log_form=True, k_seeds=0, index_offset=0, return_values=False):
        self.calls.append(("cehvi_argbest", int(np.shape(cell_lo)[0]), len(lb), bool(log_form)))
        rows = [np.asarray(r)[:int(np.argmax(np.isposinf(r))) + 1] for r in levels]
        n = len(rows) + len(lb)
        mu, sd = np.stack([self.post[j][0] for j in range(n)]), np.stack([self.post[j][1] for j in range(n)])
        self.cehvi = CM.cehvi_keys(mu, sd, rows, (cell_lo, cell_hi), lb, ub, log_form)
        bi, bv, si, sv = ET.argbest(self.cehvi, k_seeds, index_offset)
        return bi, bv, si, sv, (self.cehvi if return_values else None)


CONSTRAINTS = [(-0.3, INF), (-INF, 1.2)]


def _constraint_values(X):
    return np.column_stack([np.sin(2.0 * X[:, 0]) - 0.5 * X[:, 1], X[:, 2] + 0.2 * X[:, 0]])


def _constrained(n=14, seed=3, engine=None, constraints=CONSTRAINTS, make=EhviEngine, **kw):
    eng = make() if engine is None else engine
    opt = ParetoOptimizer(EH.BOUNDS, 2, np.full(2, -1.5), n_restarts_optimizer=2, random_state=seed, engine=eng,
                          constraints=constraints, **kw)
    for gp in opt._gps + opt._cgps:
        gp.lml_on_device = False
    lo, hi = np.array(list(EH.BOUNDS.values())).T
    X = lo + np.random.RandomState(0).uniform(size=(n, 3)) * (hi - lo)
    for x, y, c in zip(X, EH._objectives(X, 2), _constraint_values(X)[:, :len(constraints)]):
        opt.register(dict(zip(EH.BOUNDS, x)), y, c)
    return opt, eng


def test_constrained_suggest_calls_randomstate_front_and_info():
    M = 400
    opt, eng = _constrained()
    feas = opt.feasible
    assert feas.dtype == bool and 0 < feas.sum() < len(opt)
    assert np.array_equal(feas, np.all((opt.constraint_values >= [-0.3, -INF]) & (opt.constraint_values <= [INF, 1.2]), axis=1))
    X, Y = opt.front
    assert np.array_equal(Y, pareto_front(opt.targets[feas], opt.ref_point)) and opt.hypervolume == hypervolume(opt.targets[feas],
                                                                                                               opt.ref_point)
    assert opt.hypervolume < hypervolume(opt.targets, opt.ref_point), "the infeasible observations held a part of the front"
    params, info = opt.suggest(n_random=M, return_info=True)
    names = [c[0] for c in eng.calls]
    assert names[0] == "overlapped_fits" and [c[1] for c in eng.calls if c[0] == "fit"] == [0, 1, 2, 3]
    assert names.count("generate_candidates_like") == 1 and [c[1] for c in eng.calls if c[0] == "posterior"] == [0, 1, 2, 3]
    last_fit = max(i for i, c in enumerate(names) if c in ("fit", "lml", "lml_batch"))
    assert last_fit < names.index("generate_candidates_like") < names.index("posterior") < names.index("cehvi_argbest")
    assert names[-1] == "cehvi_argbest" and names.count("cehvi_argbest") == 1 and "ehvi_argbest" not in names
    assert eng.calls[-1][2:] == (2, True)
    # the RandomState: the objectives' theta searches, then the constraints', in slot order, then the candidate draw
    twin, teng = _constrained()
    for j, gp in enumerate(twin._gps):
        gp.fit(twin.params, twin.targets[:, j])
    for j, gp in enumerate(twin._cgps):
        gp.fit(twin.params, twin.constraint_values[:, j])
    teng.generate_candidates_like(M, twin.bounds[:, 0], twin.bounds[:, 1], twin._random_state)
    assert B.same_state(opt._random_state, twin._random_state) and np.array_equal(eng.Xc, teng.Xc)
    assert [gp.slot for gp in opt._cgps] == [2, 3] and all(gp.random_state is opt._random_state for gp in opt._cgps)
    # the boxes are the feasible front's; the value is log E + s at the pick
    assert info["front_size"] == Y.shape[0] and info["n_cells"] == box_decomposition(Y, opt.ref_point)[2].shape[0]
    assert info["index"] == int(np.argmin(eng.cehvi)) and info["value"] == -eng.cehvi.min() and np.isfinite(info["value"])
    assert np.array_equal(np.array(list(params.values())), eng.Xc[info["index"]])


def test_no_feasible_observation_gives_the_one_box_above_the_reference_point():
    opt, eng = _constrained(constraints=[(50.0, INF)])
    assert not opt.feasible.any() and opt.front[1].shape == (0, 2) and opt.hypervolume == 0.0
    _params, info = opt.suggest(n_random=200, return_info=True)
    assert info["front_size"] == 0 and info["n_cells"] == 1 and eng.calls[-1][:2] == ("cehvi_argbest", 1)


def test_constraints_none_is_call_for_call_what_it_was():
    plain, eng = EH._optimizer(2)
    none, eng_none = EH._optimizer(2, constraints=None)
    assert plain.suggest(n_random=300) == none.suggest(n_random=300)
    assert [c[0] for c in eng.calls] == [c[0] for c in eng_none.calls] and "cehvi_argbest" not in [c[0] for c in eng.calls]
    assert B.same_state(plain._random_state, none._random_state)
    assert none.constraints is None and none._cgps == [] and none.feasible.all() and none.constraint_values.shape == (len(none), 0)
    assert np.array_equal(none.front[1], pareto_front(none.targets, none.ref_point))
    with pytest.raises(ValueError, match="no constraints"):
        none.register({"a": 0.1, "b": 0.0, "c": 1.0}, [0.0, 0.0], [1.0])


def test_constrained_refusals():
    for bad in ([], [(1.0, 1.0)], [(2.0, 1.0)], [(np.nan, 1.0)], [1.0], "ab"):
        with pytest.raises(ValueError, match="constraints"):
            ParetoOptimizer(EH.BOUNDS, 2, np.zeros(2), constraints=bad)
    with pytest.raises(ValueError, match="must not exceed 8"):
        ParetoOptimizer(EH.BOUNDS, 2, np.zeros(2), constraints=[(0.0, 1.0)] * 7)
    with pytest.raises(ValueError, match="must not exceed 8"):
        ParetoOptimizer(EH.BOUNDS, 3, np.zeros(3), constraints=[(0.0, 1.0)] * 6)
    assert len(ParetoOptimizer(EH.BOUNDS, 3, np.zeros(3), constraints=[(0.0, 1.0)] * 5, engine=EhviEngine())._cgps) == 5
    opt, eng = _constrained(n=0)
    for bad in (None, [0.0], [0.0, np.nan], [0.0, 1.0, 2.0]):
        with pytest.raises(ValueError, match="constraint_values"):
            opt.register({"a": 0.1, "b": 0.0, "c": 1.0}, [0.0, 0.0], bad)
    with pytest.raises(A.TargetSpaceEmptyError):
        opt.suggest()
    # an engine without the call
    opt, eng = _constrained(make=EH.EhviFakeEngine)
    with pytest.raises(NotImplementedError, match="cehvi_argbest"):
        opt.suggest(n_random=50)
    assert "fit" not in [c[0] for c in eng.calls]


# ---- suggest_constrained_qnehvi over the engine double ------------------------------------------------------------------------------
class BatchEngine(QH.Engine):
    def cnehvi_greedy(self, draws, q, lb, ub, ref, base=None, y_mean=None, y_std=None, index_offset=0, return_values=False,
                      return_keys=False, return_fronts=False):
        draws = [list(g) for g in draws]
        G, S = len(draws[0]), np.shape(draws[0][0][2])[0]
        self.calls.append(("cnehvi_greedy", len(draws) - 2, G, S, int(q)))
        base = np.empty((0, self.Xc.shape[1])) if base is None else np.asarray(base, dtype=np.float64)
        self.cnehvi_args = dict(draws=draws, lb=np.array(lb), ub=np.array(ub), ref=np.array(ref), base=np.array(base),
                                y_mean=list(y_mean), y_std=list(y_std))
        pts = np.vstack([self.Xc, base])
        vals = np.array([Q.group_values(Q.P.paths_cho, self.inputs[j][1], self.inputs[j][0], self.targets[j], self.inputs[j][2],
                                        self.inputs[j][3], draws[j], pts, y_mean[j], y_std[j]) for j in range(len(draws))])
        M = self.Xc.shape[0]
        out = CM.rule(vals[:, :, :M], vals[:, :, M:], np.asarray(lb), np.asarray(ub), np.asarray(y_std), ref, int(q), index_offset)
        self.cnehvi_out = out
        size = np.array([[f.shape[0] for f in out["fronts_before"]], [f.shape[0] for f in out["fronts_after"]]], dtype=np.int32)
        return {"index": out["index"], "gain": out["gain"], "feasible": out["feasible"], "values": None, "viol": None,
                "base_values": None, "keys": None, "front_size": size if return_fronts else None, "fronts": None}


@pytest.mark.parametrize("n_draws,with_pending", [(10, False), (20, True)])
def test_batch_picks_calls_randomstate_and_info(n_draws, with_pending):
    n_features, q, M, N, D = 32, 4, 63, 14, 3
    opt, eng = _constrained(make=BatchEngine)
    lo, hi = opt.bounds[:, 0], opt.bounds[:, 1]
    pend = lo + np.random.RandomState(4).uniform(size=(2, D)) * (hi - lo) if with_pending else None
    picks, info = suggest_constrained_qnehvi(opt, q, n_random=M, n_draws=n_draws, n_features=n_features, pending=pend, return_info=True)
    G, S = draw_layout(n_draws)
    names = [c[0] for c in eng.calls]
    assert names[0] == "overlapped_fits" and [c[1] for c in eng.calls if c[0] == "fit"] == [0, 1, 2, 3]
    assert names.count("generate_candidates_like") == 1 and names.count("cnehvi_greedy") == 1
    assert [c for c in eng.calls if c[0] == "cnehvi_greedy"][0][1:] == (2, G, S, q)
    assert not {"sample_paths", "posterior", "acq_argbest", "ehvi_argbest", "cehvi_argbest", "qnehvi_greedy", "set_candidates"} & set(names)
    # the RandomState: a twin's four fits and candidate draw, then per GROUP the four slots in slot order
    twin, teng = _constrained(make=BatchEngine)
    gps = twin._gps + twin._cgps
    for gp, y in zip(gps, list(twin.targets.T) + list(twin.constraint_values.T)):
        gp.fit(twin.params, y)
    rng = twin._random_state
    teng.generate_candidates_like(M, lo, hi, rng)
    assert np.array_equal(teng.Xc, eng.Xc)
    for g in range(G):
        for j, gp in enumerate(gps):
            omega, phase = spectral_draw(gp._kind, n_features, D, rng)
            w = rng.standard_normal((S, n_features))
            eps = rng.standard_normal((S, N)) * np.sqrt(float(gp.alpha))
            assert all(np.array_equal(a, b) for a, b in zip(eng.cnehvi_args["draws"][j][g], (omega, phase, w, eps)))
    assert B.same_state(opt._random_state, rng)
    a = eng.cnehvi_args
    assert np.array_equal(a["ref"], opt.ref_point) and np.array_equal(a["lb"], [-0.3, -INF]) and np.array_equal(a["ub"], [INF, 1.2])
    assert np.array_equal(a["base"], opt.params if pend is None else np.vstack([opt.params, pend])), "ALL observed params, then pending"
    every = opt._gps + opt._cgps
    assert a["y_mean"] == [float(gp._y_train_mean) for gp in every] and a["y_std"] == [float(gp._y_train_std) for gp in every]
    out = eng.cnehvi_out
    assert set(info) == {"gain", "index", "feasible", "front_size_before", "front_size_after", "n_draws"} and info["n_draws"] == G * S
    assert np.array_equal(info["index"], out["index"]) and np.array_equal(info["gain"], out["gain"])
    assert np.array_equal(info["feasible"], out["feasible"])
    assert info["front_size_before"] == max(f.shape[0] for f in out["fronts_before"])
    assert info["front_size_after"] == max(f.shape[0] for f in out["fronts_after"])
    assert np.array_equal(np.array([list(p.values()) for p in picks]), eng.Xc[out["index"]]) and all(list(p) == opt.keys for p in picks)


def test_batch_refusals_in_their_order():
    from bayesianoptimization_amd.engine import GroupEngine

    opt, eng = _constrained(make=BatchEngine)
    for bad in (0, 65, 1.5, True):
        with pytest.raises(ValueError, match="q must be an integer"):
            suggest_constrained_qnehvi(opt, bad)
    with pytest.raises(ValueError, match="pending"):
        suggest_constrained_qnehvi(opt, 2, pending=np.zeros((2, 2)))
    three = ParetoOptimizer(EH.BOUNDS, 3, np.zeros(3), engine=BatchEngine(), constraints=[(0.0, 1.0)])
    with pytest.raises(NotImplementedError, match="3 objectives"):
        suggest_constrained_qnehvi(three, 2)
    plain, _ = QH._optimizer()
    with pytest.raises(ValueError, match="use suggest_qnehvi"):
        suggest_constrained_qnehvi(plain, 2)
    empty, _ = _constrained(n=0, make=BatchEngine)
    with pytest.raises(A.TargetSpaceEmptyError):
        suggest_constrained_qnehvi(empty, 2)
    group = object.__new__(GroupEngine)
    group.__dict__.update(_g=None, _h=None)
    grouped, _ = _constrained(engine=group)
    with pytest.raises(NotImplementedError, match="device group"):
        suggest_constrained_qnehvi(grouped, 2)
    from sklearn.gaussian_process.kernels import RationalQuadratic

    hosted, heng = _constrained(make=BatchEngine, kernel=RationalQuadratic())
    with pytest.raises(NotImplementedError, match="runs on the host"):
        suggest_constrained_qnehvi(hosted, 2)
    lacking, _ = _constrained(make=EhviEngine)
    with pytest.raises(NotImplementedError, match="no cnehvi_greedy"):
        suggest_constrained_qnehvi(lacking, 2)
    assert not eng.calls and not heng.calls
    with contextlib.suppress(Exception):
        group.__dict__.clear()
