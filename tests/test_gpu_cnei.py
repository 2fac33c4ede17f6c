"""GPU (-m gpu): gpbo_cnei_greedy — greedy batch noisy expected improvement under constraints over a resident (T, M) block of MASKED
posterior draws — against tests/cnei_truth.py.

Parity: values_out and base_values_out per slot against paths_truth at tests/test_gpu_qnei.py's norm and bar — max(1e-9, 8 x the
spread of the two NumPy routes) —; feasibility (viol == 0) against the truth's outside the pairs whose truth constraint value is
within bar x scale of a bound (tests/test_cqnei_host.py caps their share on the truth alone).
Same bits as gpbo_sample_paths_constrained: rows [g S, (g + 1) S) of values_out[j] and of viol_out are that call's values_out[j] and
viol_out for group g's inputs.
Exact replay: from the device's OWN values_out, base_values_out and baseline_out the truth reproduces viol's zero pattern (the mask),
m_t, keys_out bit for bit, and pick_idx / pick_gain / pick_feasible exactly — for q = min(8, M), q = M = 5 through the zero-gain tail,
and q = 64.
Equivalence with plain qNEI: every bound infinite, base = the pending points, y_floor = y_best: gpbo_qnei_greedy(noisy = 0)'s bits.
The shapes are cnei_truth.CASES: the edges of the code, not the workload."""
import numpy as np
import pytest

import batch_truth as B
import cnei_truth as CT
import qnei_truth as Q
from bayesianoptimization_amd import _lib
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd import suggest_constrained_qnei
from bayesianoptimization_amd._lib import GpboError, dptr, iptr
from bayesianoptimization_amd.constraint_model import HipConstraintModel
from bayesianoptimization_amd.engine import GpEngine, GroupEngine
from bayesianoptimization_amd.float_space import FloatSpace
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

INF = np.inf
SMALL = "c1-n65,64-m63-f64-d2-2x5-b66"
BIG = "c2-n130,65,64-m514-f65-d5-3x16-b194"


@pytest.fixture(scope="module")
def engine():
    """A context of this module's own: its cases fit every slot up to 7, and the suite's shared context has tests that count on
    slots nobody has fitted."""
    eng = GpEngine(0)
    yield eng
    eng.close()


def replay(c, out, q, what, lb=None, ub=None, y_floor=None, index_offset=0):
    """the truth's rule on the device's own raw values: the mask, m_t, the keys bit for bit, picks, gains and shares exactly"""
    lb = c.lb if lb is None else np.asarray(lb, dtype=np.float64)
    ub = c.ub if ub is None else np.asarray(ub, dtype=np.float64)
    y_floor = c.y_floor if y_floor is None else y_floor
    t = CT.rule(out["values"], out["base_values"], lb, ub, c.y_std, y_floor, q, index_offset)
    viol = out["viol"]
    assert np.array_equal(viol == 0.0, t["viol"] == 0.0) and np.array_equal(np.isnan(viol), np.isnan(t["viol"])), f"{what}: the mask"
    assert np.array_equal(out["baseline"], t["baseline"], equal_nan=True), f"{what}: m_t"
    keys = out["keys"]
    assert keys.shape == (q, out["values"].shape[2])
    assert np.array_equal(keys, t["keys"], equal_nan=True), f"{what}: keys differ at {np.argwhere(~((keys == t['keys']) | (np.isnan(keys) & np.isnan(t['keys']))))[:4].tolist()}"
    assert np.array_equal(out["index"], t["index"]), f"{what}: picks {out['index'].tolist()}, replay {t['index'].tolist()}"
    assert np.array_equal(out["gain"], t["gain"], equal_nan=True) and not np.signbit(out["gain"][out["gain"] == 0.0]).any()
    assert np.array_equal(out["feasible"], t["feasible"], equal_nan=True), f"{what}: shares {out['feasible'].tolist()}, replay {t['feasible'].tolist()}"
    return t


# ---- parity and the replay, case by case -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CT.CASES))
def test_parity_and_exact_replay(engine, name):
    c = CT.case_of(name)
    c.fit(engine)
    q = min(8, c.M)
    out = c.run(engine, q)
    assert out["values"].shape == (1 + c.C, c.T, c.M) and out["viol"].shape == (c.T, c.M) and out["baseline"].shape == (c.T,)
    assert out["base_values"].shape == (1 + c.C, c.T, c.B)
    for j in range(1 + c.C):
        e = c.err_of(out["values"][j], c.ref[j][:, :c.M], j)
        eb = c.err_of(out["base_values"][j], c.ref[j][:, c.M:], j) if c.B else 0.0
        print(f"{c.what} slot {j}: values {e:.2e}, base values {eb:.2e}, bar {c.bars[j]:.2e} (the reference's own {c.own[j]:.2e})")
        assert e <= c.bars[j] and eb <= c.bars[j], f"{c.what} slot {j}: error {max(e, eb):.2e} over its bar {c.bars[j]:.2e}"
    t = replay(c, out, q, c.what)
    # feasibility against the truth, outside the pairs next to a bound
    truth = c.truth(q)
    far = ~c.near_a_bound()
    got = np.hstack([t["masked"], t["masked_base"]]) > -INF
    want = np.hstack([truth["masked"], truth["masked_base"]]) > -INF
    assert np.array_equal(got[far], want[far]), f"{c.what}: feasibility differs from the truth's away from the bounds"
    if c.B == 0:
        assert np.array_equal(out["baseline"], np.full(c.T, c.y_floor))
    if name == CT.FLOOR_CASE:
        none = ~(t["masked_base"] > -INF).any(axis=1)
        assert none.any() and not none.all() and np.array_equal(out["baseline"][none], np.full(none.sum(), c.y_floor))
    # nothing asked for: the same picks
    lean = c.run(engine, q, return_values=False, return_keys=False)
    assert lean["values"] is None and lean["viol"] is None and lean["keys"] is None
    for k in ("index", "gain", "feasible", "baseline"):
        assert np.array_equal(lean[k], out[k], equal_nan=True), k


@pytest.mark.parametrize("name", CT.PICK_CASES)
def test_leading_picks_against_the_truth(engine, name):
    c = CT.case_of(name)
    q = 8
    t = c.truth(q)
    g = t["masked"]
    n, gaps = Q.leading_separated_steps(np.where(np.isfinite(g), g, np.nan), t["keys"], B.GAP_FLOOR)
    print(f"{c.what}: truth picks {t['index'].tolist()}, gaps {['%.1e' % x for x in gaps]}: {n} leading separated steps")
    assert n >= 2
    c.fit(engine)
    out = c.run(engine, q)
    assert np.array_equal(out["index"][:n], t["index"][:n]), f"{c.what}: picks {out['index'][:n].tolist()}, truth {t['index'][:n].tolist()}"
    assert np.allclose(out["gain"][:n], t["gain"][:n], rtol=0.0, atol=2 * c.bars[0] * c.scale(0))


# ---- the same bits as the constrained sampler ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [BIG, "c7-n64-m63-f63-d3-1x1-b0", "c1-n64-m63-f64-d3-16x16-b66"])      # (the last: an F32 objective slot)
def test_same_bits_as_sample_paths_constrained(engine, name):
    c = CT.case_of(name)
    c.fit(engine)
    out = c.run(engine, 2)
    for g in range(c.G):
        rows = slice(g * c.S, (g + 1) * c.S)
        one = engine.sample_paths_constrained([c.draws[j][g] for j in range(1 + c.C)], c.lb, c.ub, c.y_mean, c.y_std, return_values=True)
        for j in range(1 + c.C):
            assert np.array_equal(out["values"][j][rows], one[4][j]), f"group {g} slot {j}: not gpbo_sample_paths_constrained's values"
        assert np.array_equal(out["viol"][rows], one[5]), f"group {g}: not gpbo_sample_paths_constrained's viol_out"


# ---- the exact replay at the other batch sizes -----------------------------------------------------------------------------------------
def test_replay_q_equals_m_and_q_64(engine):
    c = CT.case_of(SMALL)
    c.fit(engine)
    engine.set_candidates(c.Xc[:5])                                       # q = M = 5: every candidate once, through the zero-gain tail
    out = c.run(engine, 5)
    replay(c, out, 5, "q = M = 5")
    assert sorted(out["index"].tolist()) == [0, 1, 2, 3, 4]
    zero = out["gain"] == 0.0
    assert zero.any() and (np.diff(out["index"][zero]) > 0).all() and (out["gain"][~zero] > 0.0).all()
    with pytest.raises(ValueError, match="q exceeds"):
        c.run(engine, 6)
    engine.set_candidates(np.vstack([c.Xc, c.Xc[:1] * 0.5]))              # q = M = 64 (even: two candidates per thread)
    out = c.run(engine, 64)
    replay(c, out, 64, "q = M = 64")
    assert sorted(out["index"].tolist()) == list(range(64))
    big = CT.case_of(BIG)
    big.fit(engine)
    out = big.run(engine, 64)
    replay(big, out, 64, "q = 64 of 514")
    assert len(set(out["index"].tolist())) == 64 and (np.diff(out["gain"]) <= 0.0).all()


# ---- equivalence with plain qNEI ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [SMALL, BIG])
def test_infinite_bounds_are_plain_qnei(engine, name):
    c = CT.case_of(name)
    c.fit(engine)
    pending = c.base[-2:]
    y_best = float(np.median(c.ref[0]))
    q = 8
    out = c.run(engine, q, lb=np.full(c.C, -INF), ub=np.full(c.C, INF), y_floor=y_best, base=pending)
    idx, gain, m0, values, keys = engine.qnei_greedy(c.draws[0], q, noisy=False, y_best=y_best, pending=pending, y_mean=c.y_mean[0],
                                                     y_std=c.y_std[0], return_values=True, return_keys=True)
    assert np.array_equal(out["values"][0], values) and np.array_equal(out["baseline"], m0) and np.array_equal(out["keys"], keys)
    assert np.array_equal(out["index"], idx) and np.array_equal(out["gain"], gain)
    assert (out["feasible"] == 1.0).all() and (out["viol"] == 0.0).all()


# ---- conventions ----------------------------------------------------------------------------------------------------------------------
def test_nan_infeasible_pick_offset_and_repeatable(engine):
    c = CT.case_of(SMALL)
    c.fit(engine)
    base = c.run(engine, 6)
    again = c.run(engine, 6)
    for k in base:                                                       # bitwise repeatable
        assert np.array_equal(base[k], again[k], equal_nan=True), k
    off = c.run(engine, 6, index_offset=10**10)                          # index_offset is added, nothing else changes
    assert np.array_equal(off["index"], base["index"] + 10**10)
    for k in ("gain", "feasible", "baseline", "keys", "values", "viol"):
        assert np.array_equal(off[k], base[k], equal_nan=True), k
    replay(c, off, 6, "index_offset", index_offset=10**10)
    # a NaN candidate: NaN in every slot's draws there, it takes the first pick with a NaN gain and a NaN share, is masked from
    # step 1 on, leaves every incumbent as it was, and the later steps are the greedy's
    k = next(i for i in range(c.M - 1, -1, -1) if i not in base["index"][:3])
    Xn = c.Xc.copy()
    Xn[k, 1] = np.nan
    engine.set_candidates(Xn)
    out = c.run(engine, 4)
    assert out["index"][0] == k and np.isnan(out["gain"][0]) and np.isnan(out["feasible"][0]) and out["keys"][1][k] == INF
    assert np.isnan(out["viol"][:, k]).all() and np.array_equal(out["baseline"], base["baseline"])
    assert np.array_equal(out["index"][1:], base["index"][:3]) and np.array_equal(out["gain"][1:], base["gain"][:3])
    assert np.array_equal(out["feasible"][1:], base["feasible"][:3])
    replay(c, out, 4, "a NaN candidate")
    engine.set_candidates(c.Xc)
    # a NaN constraint value at a base point (through one constraint weight of group 0: that draw's constraint is NaN everywhere):
    # the fold drops it, so the draw starts from y_floor; every candidate's key is NaN, the lowest unmasked index wins each step
    om, ph, w, eps = c.draws[1][0]
    wn = w.copy()
    wn[2, 5] = np.nan
    draws = [c.draws[0], [(om, ph, wn, eps)] + c.draws[1][1:]]
    out = c.run(engine, 3, draws=draws)
    assert np.isnan(out["base_values"][1][2]).all() and np.isnan(out["viol"][2]).all() and out["baseline"][2] == c.y_floor
    assert np.array_equal(np.delete(out["baseline"], 2), np.delete(base["baseline"], 2))
    assert out["index"].tolist() == [0, 1, 2] and np.isnan(out["gain"]).all() and np.isnan(out["feasible"]).all()
    replay(c, out, 3, "a NaN constraint draw")
    # an infeasible pick leaves every m_t unchanged: with q = M every candidate is picked, among them one that NO draw calls feasible
    # (asserted on the device's own mask), and the final incumbents are the fold of the feasible values alone
    f = CT.case_of(CT.FLOOR_CASE)
    f.fit(engine)
    out = f.run(engine, 63)
    t = replay(f, out, 63, "q = M = 63, the floor case")
    dead = ~(t["masked"] > -INF).any(axis=0)
    assert dead.any() and (out["feasible"][np.isin(out["index"], np.flatnonzero(dead))] == 0.0).all()
    assert (out["gain"][out["feasible"] == 0.0] == 0.0).all()
    j = int(np.flatnonzero(np.isin(out["index"], np.flatnonzero(dead)))[0])      # the first such pick: the next step's keys are this
    live = out["keys"][j + 1] != INF                                             # step's for every candidate still unpicked
    assert j + 1 < 63 and np.array_equal(out["keys"][j][live], out["keys"][j + 1][live])


# ---- a reader -------------------------------------------------------------------------------------------------------------------------
def test_reader_only(engine):
    eng = engine
    c = CT.case_of(BIG)
    plain = CT.Case(**{**CT.CASES[BIG], "scaled_slot": None}).references()      # (unscaled slots: fit_append below)
    plain.fit(eng)
    for j in range(1 + c.C):
        eng.posterior(j, plain.y_mean[j], plain.y_std[j], fetch=False)
    eng.take_negative_variance_flag()
    before = eng.acq_argbest(O.UCB, 2.576, k_seeds=8, return_values=True)
    mu_sd = [eng.posterior(j, plain.y_mean[j], plain.y_std[j]) for j in range(1 + c.C)]
    plain.run(eng, 8)
    after = eng.acq_argbest(O.UCB, 2.576, k_seeds=8, return_values=True)      # still answers, from the posterior before the call
    assert before[0] == after[0] and before[1] == after[1] and np.array_equal(before[2], after[2])
    assert np.array_equal(before[3], after[3]) and np.array_equal(before[4], after[4])
    assert np.array_equal(eng.get_candidate_rows(np.arange(c.M), c.d), plain.Xc)
    assert eng.take_negative_variance_flag() is False
    for j in range(1 + c.C):                                                  # the fits answer as before
        mu, sd = eng.posterior(j, plain.y_mean[j], plain.y_std[j])
        assert np.array_equal(mu, mu_sd[j][0]) and np.array_equal(sd, mu_sd[j][1])
    # an append to a constraint slot, the greedy over the grown model, and the refresh still takes its incremental route
    s = plain.slots[1]
    x_new = np.random.RandomState(5).uniform(size=(2, c.d))
    yn2 = np.concatenate([s["yn"], [0.2, -0.4]])
    draws2 = [plain.draws[0], [(om, ph, w, np.hstack([eps, np.zeros((plain.S, 2))])) for om, ph, w, eps in plain.draws[1]], plain.draws[2]]

    def arm():
        plain.fit(eng)
        eng.posterior(1, plain.y_mean[1], plain.y_std[1], fetch=False)
        eng.fit_append(x_new, yn2, slot=1)

    arm()
    mu_a, sd_a, route_a = eng.posterior_refresh(1, plain.y_mean[1], plain.y_std[1], return_route=True)
    arm()
    plain.run(eng, 8, draws=draws2)
    mu_b, sd_b, route_b = eng.posterior_refresh(1, plain.y_mean[1], plain.y_std[1], return_route=True)
    assert route_a == 1 and route_b == 1
    assert np.array_equal(mu_a, mu_b) and np.array_equal(sd_a, sd_b)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals(engine):
    eng = engine
    c = CT.case_of(SMALL)
    c.fit(eng)
    G, S, Fn, d, C = c.G, c.S, c.F, c.d, c.C
    flat = [t for groups in c.draws for t in groups]
    omega = np.ascontiguousarray(np.concatenate([t[0].ravel() for t in flat]))
    phase = np.ascontiguousarray(np.concatenate([t[1] for t in flat]))
    w = np.ascontiguousarray(np.concatenate([t[2].ravel() for t in flat]))
    eps = np.ascontiguousarray(np.concatenate([t[3].ravel() for t in flat]))
    base = np.ascontiguousarray(c.base)
    y_mean, y_std = np.ascontiguousarray(c.y_mean), np.ascontiguousarray(c.y_std)
    lb, ub = np.ascontiguousarray(c.lb), np.ascontiguousarray(c.ub)
    pi, pg, pf, bl = np.empty(64, dtype=np.int64), np.empty(64), np.empty(64), np.empty(256)

    def call(h=None, n_constraints=C, ym=y_mean, ys=y_std, lo=lb, hi=ub, n_groups=G, n_paths=S, n_features=Fn, draws=None,
             y_floor=c.y_floor, bp=dptr(base), n_base=c.B, dd=d, q=4, outs=None, frames=None):
        draws = [dptr(omega), dptr(phase), dptr(w), dptr(eps)] if draws is None else draws
        outs = [iptr(pi), dptr(pg), dptr(pf), dptr(bl)] if outs is None else outs
        frames = [dptr(ym), dptr(ys), dptr(lo), dptr(hi)] if frames is None else frames
        return eng._lib.gpbo_cnei_greedy(eng._h if h is None else h, n_constraints, *frames, n_groups, n_paths, n_features, *draws,
                                         y_floor, bp, n_base, dd, q, 0, *outs, None, None, None, None)

    assert call() == _lib.GPBO_OK
    # n_constraints outside [1, GPBO_MAX_MODELS - 1]; n_groups, n_paths, n_features outside their ranges
    assert call(n_constraints=0) == _lib.ERR_INVALID and call(n_constraints=8) == _lib.ERR_INVALID
    assert call(n_groups=0) == _lib.ERR_INVALID and call(n_groups=17) == _lib.ERR_INVALID
    assert call(n_paths=0) == _lib.ERR_INVALID and call(n_paths=17) == _lib.ERR_INVALID
    assert call(n_features=0) == _lib.ERR_INVALID and call(n_features=4097) == _lib.ERR_INVALID
    # a NULL among y_mean / y_std / lb / ub, the draw inputs, pick_idx / pick_gain / pick_feasible / baseline_out
    for k in range(4):
        a = [dptr(y_mean), dptr(y_std), dptr(lb), dptr(ub)]
        a[k] = None
        assert call(frames=a) == _lib.ERR_INVALID
        a = [dptr(omega), dptr(phase), dptr(w), dptr(eps)]
        a[k] = None
        assert call(draws=a) == _lib.ERR_INVALID
        a = [iptr(pi), dptr(pg), dptr(pf), dptr(bl)]
        a[k] = None
        assert call(outs=a) == _lib.ERR_INVALID
    # a y_std not finite or not positive, a y_mean not finite, in either slot
    for j in range(1 + C):
        for bad in (0.0, -1.0, np.inf, np.nan):
            v = y_std.copy()
            v[j] = bad
            assert call(ys=v) == _lib.ERR_INVALID
        for bad in (np.inf, np.nan):
            v = y_mean.copy()
            v[j] = bad
            assert call(ym=v) == _lib.ERR_INVALID
    # a NaN bound, lb >= ub; infinite sides are allowed
    assert call(lo=np.array([np.nan])) == _lib.ERR_INVALID and call(hi=np.array([np.nan])) == _lib.ERR_INVALID
    assert call(lo=ub.copy(), hi=ub.copy()) == _lib.ERR_INVALID and call(lo=ub.copy(), hi=lb.copy()) == _lib.ERR_INVALID
    assert call(lo=np.array([-INF]), hi=np.array([INF])) == _lib.GPBO_OK
    # y_floor not finite
    for bad in (np.inf, -np.inf, np.nan):
        assert call(y_floor=bad) == _lib.ERR_INVALID
    # n_base outside [0, GPBO_MAX_CNEI_BASE], n_base > 0 with a NULL or non-finite base, d not the slots'
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
    # the engine's own refusals, as exceptions
    with pytest.raises(ValueError, match="1 \\+ C lists"):
        eng.cnei_greedy(c.draws[:1], 2, c.lb, c.ub, 0.0)
    with pytest.raises(ValueError, match="n_groups"):
        eng.cnei_greedy([g * 9 for g in c.draws], 2, c.lb, c.ub, 0.0)
    with pytest.raises(ValueError, match="same non-empty list"):
        eng.cnei_greedy([c.draws[0], c.draws[1][:1]], 2, c.lb, c.ub, 0.0)
    with pytest.raises(ValueError, match="lb / ub"):
        eng.cnei_greedy(c.draws, 2, [0.0, 1.0], [1.0, 2.0], 0.0)
    with pytest.raises(ValueError, match="base"):
        eng.cnei_greedy(c.draws, 2, c.lb, c.ub, 0.0, base=np.zeros((1, d + 1)))
    with pytest.raises(ValueError, match="q out of range"):
        c.run(eng, 65)
    with pytest.raises(ValueError, match="y_floor"):
        c.run(eng, 2, y_floor=np.nan)
    # GPBO_ERR_STATE: a constraint slot that gpbo_lml left unfitted
    s = c.slots[1]
    eng.lml(s["X"], s["yn"], s["kind"], s["ls"], CT.NOISE, slot=1)
    with pytest.raises(GpboError, match="not been fitted"):
        c.run(eng, 2)
    assert call() == _lib.ERR_STATE
    c.fit(eng)
    # ... a fit pending on a slot (the engine would wait for it: asked at the C boundary)
    with eng.overlapped_fits():
        eng.fit(s["X"], s["yn"], s["kind"], s["ls"], CT.NOISE, slot=1)
        assert call() == _lib.ERR_STATE
    assert call() == _lib.GPBO_OK
    # ... candidates of another d
    eng.set_candidates(np.random.RandomState(1).uniform(size=(10, d + 1)))
    with pytest.raises(GpboError, match="dimension"):
        c.run(eng, 2)
    # ... no resident candidates: a context that never had any
    fresh = GpEngine(0)
    try:
        assert call(h=fresh._h) == _lib.ERR_STATE
        for j, sl in enumerate(c.slots):
            fresh.fit(sl["X"], sl["yn"], sl["kind"], sl["ls"], CT.NOISE, slot=j)
        with pytest.raises(GpboError, match="no candidates"):
            c.run(fresh, 2)
    finally:
        fresh.close()
    # a device group
    with pytest.raises(NotImplementedError, match="device group"):
        GroupEngine.cnei_greedy(object.__new__(GroupEngine), c.draws, 2, c.lb, c.ub, 0.0)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def test_suggest_constrained_qnei_picks_the_replays_picks(engine, monkeypatch):
    D, N, M, q, n_draws, FEATURES = 3, 30, 257, 4, 20, 128
    bounds = np.array([[0.0, 1.0]] * D)
    X = np.random.RandomState(130).uniform(size=(N, D))
    y = np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1]) + X[:, 2] ** 2 + 0.05 * np.random.RandomState(131).standard_normal(N)
    cvals = np.cos(X.sum(1)) + 0.05 * np.random.RandomState(132).standard_normal(N)
    drv = B.Driver(engine, X, y, bounds, A.UpperConfidenceBound(kappa=2.576), seed=7, n_random=M)
    cm = HipConstraintModel(None, np.array([-INF]), np.array([0.5]), engine=engine, random_state=np.random.RandomState(3))
    drv._space = FloatSpace({f"x{j}": (0.0, 1.0) for j in range(D)}, constraint=cm)
    drv._space.register_bulk(X, y, cvals)
    seen = {}
    real = engine.cnei_greedy

    def recording(draws, q_, lb, ub, y_floor, **kw):
        kw.update(return_values=True, return_keys=True)
        seen.update(draws=draws, lb=lb, ub=ub, y_floor=y_floor, kw=kw)
        seen["out"] = real(draws, q_, lb, ub, y_floor, **kw)
        return seen["out"]

    monkeypatch.setattr(engine, "cnei_greedy", recording)
    pending = [{"x0": 0.25, "x1": 0.5, "x2": 0.75}]
    picks, info = suggest_constrained_qnei(drv, q, n_random=M, n_draws=n_draws, n_features=FEATURES, pending=pending, return_info=True)
    out = seen["out"]
    assert out["values"].shape == (2, 20, M) and out["base_values"].shape == (2, 20, N + 1) and info["n_draws"] == 20
    assert len(seen["draws"]) == 2 and len(seen["draws"][0]) == 2 and np.array_equal(seen["kw"]["base"], np.vstack([X, [[0.25, 0.5, 0.75]]]))
    assert seen["y_floor"] == y.min() - np.ptp(y) and np.array_equal(seen["lb"], [-INF]) and np.array_equal(seen["ub"], [0.5])
    t = CT.rule(out["values"], out["base_values"], np.array([-INF]), np.array([0.5]), np.asarray(seen["kw"]["y_std"]), seen["y_floor"], q)
    assert np.array_equal(out["keys"], t["keys"], equal_nan=True)
    assert np.array_equal(info["index"], t["index"]) and np.array_equal(info["gain"], t["gain"])
    assert np.array_equal(info["feasible"], t["feasible"]) and np.array_equal(info["baseline"], t["baseline"])
    Xc = engine.get_candidate_rows(np.arange(M), D)                           # the one candidate draw is still resident
    assert np.array_equal(np.array([list(p.values()) for p in picks]), Xc[t["index"]])
    assert info["gain"][0] > 0.0 and 0.0 < info["feasible"][0] <= 1.0
