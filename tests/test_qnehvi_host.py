"""CPU: greedy batch noisy expected hypervolume improvement's host side — the strip sum, the fronts and the update rule of
tests/qnehvi_truth.py against `multiobjective.hypervolume` / `pareto_front` on random and hand-made fronts (ties, duplicates, empty
fronts, points on ref, NaNs), and `suggest_qnehvi` over an oracle-backed engine double: the order of the refusals, the engine calls,
the RandomState it leaves behind, `pending`, the info dict.  The device's arithmetic is checked in tests/test_gpu_qnehvi.py."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest

import batch_truth as B
import qnehvi_truth as Q
from bayesianoptimization_amd import _lib, suggest_qnehvi
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd.multiobjective import ParetoOptimizer, hypervolume, pareto_front
from bayesianoptimization_amd.qnei import draw_layout
from bayesianoptimization_amd.thompson import spectral_draw
from conftest import ROOT

REF = np.array([-0.5, 0.25])


def _pairs(rs, n):
    """n pairs on a coarse grid around REF: ties in one objective, duplicates, points on and below ref all occur"""
    return np.column_stack([REF[0] + rs.randint(-1, 6, n) * 0.25 + rs.randint(0, 2, n) * rs.uniform(0, 1e-3, n),
                            REF[1] + rs.randint(-1, 6, n) * 0.5])


# ---- the strip sum, the fronts, the update rule -----------------------------------------------------------------------------------
def test_strip_sum_is_the_hypervolume_difference():
    """HVI(y | P) = hypervolume(Y u {y}) - hypervolume(Y).  Both sides are sums of at most ~20 products of magnitude <= 5 here, so
    they agree to a few ulps of that: 1e-13 is 100 x the worst difference seen (2e-15 over these 200 trials)."""
    rs = np.random.RandomState(0)
    worst = 0.0
    for trial in range(200):
        Y = _pairs(rs, int(rs.randint(0, 13)))
        front = Q.front_of(Y, REF)
        cands = np.vstack([_pairs(rs, 6), Y[:2], [REF], rs.uniform(-1.0, 3.0, (4, 2))])
        got = Q.hvi(cands[:, 0], cands[:, 1], front, REF)
        hv0 = hypervolume(Y, REF)
        want = np.array([hypervolume(np.vstack([Y, y[None]]), REF) - hv0 for y in cands])
        worst = max(worst, float(np.abs(got - want).max()))
        assert (got >= 0.0).all() and not np.signbit(got).any()
    print(f"worst difference {worst:.1e}")
    assert worst <= 1e-13


def test_hvi_by_hand_and_conventions():
    ref = np.array([0.0, 0.0])
    front = np.array([[3.0, 1.0], [1.0, 2.0]])
    # strips: (3, inf] x (0, inf), (1, 3] x (1, inf), (0, 1] x (2, inf)
    f0 = np.array([4.0, 2.0, 0.5, 3.0, 1.0, -1.0, np.nan, 2.0, 0.0])
    f1 = np.array([3.0, 3.0, 3.0, 1.0, 2.0, 5.0, 1.0, np.nan, 9.0])
    want = [1 * 3 + 2 * 2 + 1 * 1, 1 * 2 + 1 * 1, 0.5 * 1, 0.0, 0.0, 0.0, np.nan, np.nan, 0.0]
    assert np.array_equal(Q.hvi(f0, f1, front, ref), want, equal_nan=True)
    assert np.array_equal(Q.hvi(f0[:3], f1[:3], np.empty((0, 2)), ref), [12.0, 6.0, 1.5])      # an empty front: one strip
    # the sum runs k = 0 .. n into one accumulator, one rounded product per term
    rs = np.random.RandomState(1)
    P = Q.front_of(rs.uniform(0.1, 1.0, (40, 2)), ref)
    x, y = 0.83, 0.91
    a = np.concatenate([[np.inf], P[:, 0], [0.0]])
    c = np.concatenate([[0.0], P[:, 1]])
    acc = 0.0
    for k in range(P.shape[0] + 1):
        acc = acc + max(min(x, a[k]) - a[k + 1], 0.0) * max(y - c[k], 0.0)
    assert P.shape[0] >= 3 and Q.hvi(np.array([x]), np.array([y]), P, ref)[0] == acc
    # the keys: t = 0 .. T - 1 into one accumulator, then one division; a picked candidate is +inf
    vals = rs.uniform(0.0, 1.2, (2, 7, 5))
    fronts = [Q.front_of(rs.uniform(0.1, 1.0, (6, 2)), ref) for _ in range(7)]
    want = 0.0
    for t in range(7):
        want = want + Q.hvi(vals[0, t, 3:4], vals[1, t, 3:4], fronts[t], ref)[0]
    keys = Q.keys_of(vals, fronts, ref, np.array([False, True, False, False, False]))
    assert keys[3] == -(want / 7.0) and keys[1] == np.inf


def test_front_of_is_sorted_distinct_and_above_ref():
    nan = np.nan
    pairs = np.array([[1.0, 1.0], [2.0, 0.5], [2.0, 0.5], [0.5, 3.0], [1.0, 0.9], [nan, 9.0], [9.0, nan], [0.0, 5.0], [5.0, 0.0],
                      [2.0, 0.4], [0.5, 2.0]])
    assert Q.front_of(pairs, [0.0, 0.0]).tolist() == [[2.0, 0.5], [1.0, 1.0], [0.5, 3.0]]
    assert Q.front_of(np.empty((0, 2)), [0.0, 0.0]).shape == (0, 2) and Q.front_of([[0.0, 1.0], [-1.0, -1.0]], [0.0, 0.0]).shape == (0, 2)
    rs = np.random.RandomState(2)
    for _ in range(50):
        Y = _pairs(rs, int(rs.randint(0, 30)))
        P = Q.front_of(Y, REF)
        assert (np.diff(P[:, 0]) < 0).all() and (np.diff(P[:, 1]) > 0).all() and (P > REF).all()
        assert sorted(map(tuple, P)) == sorted(map(tuple, pareto_front(Y, REF)))


def test_insert_is_the_rebuild_from_scratch():
    rs = np.random.RandomState(3)
    for trial in range(200):
        Y = _pairs(rs, int(rs.randint(0, 12)))
        front = Q.front_of(Y, REF)
        for y in np.vstack([_pairs(rs, 5), Y[:1], [[np.nan, 1.0]], [REF]]):
            got = Q.insert(front, y, REF)
            want = Q.front_of(np.vstack([Y, y[None]]), REF)
            assert np.array_equal(got, want), (trial, front.tolist(), y.tolist())
            Y, front = np.vstack([Y, y[None]]), got
    # a full front: an insertion that dominates keeps it within the cap, one that dominates none overflows
    full = np.column_stack([np.arange(128, 0, -1.0), np.arange(1.0, 129.0)])
    assert Q.insert(full, [126.5, 5.5], [0.0, 0.0]).shape == (126, 2)       # dominates (126, 3), (125, 4), (124, 5)
    with pytest.raises(Q.FrontOverflow):
        Q.insert(full, [0.5, 200.0], [0.0, 0.0])


def test_greedy_by_hand():
    ref = np.array([0.0, 0.0])
    vals = np.array([[[2.0, 1.0, 3.0, np.nan]], [[2.0, 3.0, 1.0, 1.0]]])      # one draw, four candidates
    idx, gain, keys, fronts = Q.greedy(vals, [np.array([[1.0, 1.0]])], ref, 4, index_offset=10)
    # step 0: the NaN candidate wins; then HVI = (4 - 1, 3 - 1, 3 - 1) -> candidate 0; front (2, 2); then 1 and 2 add 1 each
    assert idx.tolist() == [13, 10, 11, 12] and np.isnan(gain[0]) and gain[1:].tolist() == [3.0, 1.0, 1.0]
    assert np.array_equal(keys[1], [-3.0, -2.0, -2.0, np.inf]) and np.array_equal(keys[2], [np.inf, -1.0, -1.0, np.inf])
    assert fronts[0].tolist() == [[3.0, 1.0], [2.0, 2.0], [1.0, 3.0]]


# ---- suggest_qnehvi over the engine double ----------------------------------------------------------------------------------------
class Engine(Q.QnehviFakeEngine):
    def overlapped_fits(self):
        self.calls.append(("overlapped_fits",))
        return contextlib.nullcontext()


BOUNDS = {"a": (0.0, 1.0), "b": (-1.0, 2.0), "c": (0.5, 1.5)}
D, N, M = 3, 14, 63


def _objectives(X, m):
    f = [np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1]) + X[:, 2] ** 2, -((X[:, 0] - 0.7) ** 2) - 0.3 * X[:, 1] + 0.2 * X[:, 2],
         np.cos(2.0 * X[:, 2]) + 0.5 * X[:, 0]]
    return np.column_stack(f[:m])


def _optimizer(m=2, n=N, seed=3, engine=None, **kw):
    eng = Engine() if engine is None else engine
    opt = ParetoOptimizer(BOUNDS, m, np.full(m, -1.5), n_restarts_optimizer=2, random_state=seed, engine=eng, **kw)
    for gp in opt._gps:
        gp.lml_on_device = False
    lo, hi = np.array(list(BOUNDS.values())).T
    X = lo + np.random.RandomState(0).uniform(size=(n, 3)) * (hi - lo)
    for x, y in zip(X, _objectives(X, m)):
        opt.register(dict(zip(BOUNDS, x)), y)
    return opt, eng


@pytest.mark.parametrize("n_draws,pending_form", [(10, None), (20, "dicts"), (33, "array")])
def test_picks_calls_randomstate_and_info(n_draws, pending_form):
    n_features, q = 32, 4
    opt, eng = _optimizer()
    lo, hi = opt.bounds[:, 0], opt.bounds[:, 1]
    pend_rows = lo + np.random.RandomState(4).uniform(size=(2, D)) * (hi - lo)
    pending = {None: None, "array": pend_rows, "dicts": [dict(zip(opt.keys, r)) for r in pend_rows]}[pending_form]
    picks, info = suggest_qnehvi(opt, q, n_random=M, n_draws=n_draws, n_features=n_features, pending=pending, return_info=True)
    G, S = draw_layout(n_draws)
    names = [c[0] for c in eng.calls]
    # the engine calls: the two fits in slot order (overlapped), one candidate draw, ONE qnehvi_greedy, one fetch of rows
    assert names[0] == "overlapped_fits" and [c[1] for c in eng.calls if c[0] == "fit"] == [0, 1]
    assert names.count("generate_candidates_like") == 1 and names.count("qnehvi_greedy") == 1
    assert [c for c in eng.calls if c[0] == "qnehvi_greedy"][0][1:] == (G, S, q)
    assert not {"sample_paths", "posterior", "posterior_refresh", "acq_argbest", "ehvi_argbest", "fit_append", "set_candidates"} & set(names)
    last_fit = max(i for i, c in enumerate(names) if c in ("fit", "lml", "lml_batch"))
    assert last_fit < names.index("generate_candidates_like") < names.index("qnehvi_greedy")
    # the RandomState: a twin's two fits and candidate draw, then objective 0's G groups, then objective 1's
    twin, teng = _optimizer()
    for j, gp in enumerate(twin._gps):
        gp.fit(twin.params, twin.targets[:, j])
    rng = twin._random_state
    teng.generate_candidates_like(M, lo, hi, rng)
    assert np.array_equal(teng.Xc, eng.Xc)
    for j, gp in enumerate(twin._gps):
        for g in range(G):
            omega, phase = spectral_draw(gp._kind, n_features, D, rng)
            w = rng.standard_normal((S, n_features))
            eps = rng.standard_normal((S, N)) * np.sqrt(float(gp.alpha))
            got = eng.qnehvi_args["draws"][j][g]
            assert all(np.array_equal(a, b) for a, b in zip(got, (omega, phase, w, eps)))
    assert B.same_state(opt._random_state, rng)
    # what the call was given
    a = eng.qnehvi_args
    assert np.array_equal(a["ref"], opt.ref_point)
    assert np.array_equal(a["base"], opt.params if pending is None else np.vstack([opt.params, pend_rows]))
    assert a["y_mean"] == [float(gp._y_train_mean) for gp in opt._gps] and a["y_std"] == [float(gp._y_train_std) for gp in opt._gps]
    # the info dict, and the picks are the greedy's on the engine's own values
    assert set(info) == {"gain", "index", "front_size_before", "front_size_after", "n_draws"} and info["n_draws"] == G * S >= n_draws
    base_values = np.stack([Q.group_values(Q.P.paths_cho, eng.inputs[j][1], eng.inputs[j][0], eng.targets[j], eng.inputs[j][2],
                                           eng.inputs[j][3], a["draws"][j], a["base"], a["y_mean"][j], a["y_std"][j]) for j in range(2)])
    f0 = Q.fronts_of(base_values, opt.ref_point)
    idx, gain, _, f1 = Q.greedy(eng.qnehvi_values, f0, opt.ref_point, q)
    assert np.array_equal(info["index"], idx) and np.array_equal(info["gain"], gain)
    assert info["front_size_before"] == max(f.shape[0] for f in f0) >= 1 and info["front_size_after"] == max(f.shape[0] for f in f1)
    assert len(picks) == q and all(list(p) == opt.keys for p in picks)
    assert np.array_equal(np.array([list(p.values()) for p in picks]), eng.Xc[idx])
    assert gain[0] > 0.0 and (np.diff(gain) <= 1e-12).all()
    again, _ = _optimizer()
    assert suggest_qnehvi(again, q, n_random=M, n_draws=n_draws, n_features=n_features, pending=pending) == picks


def test_refusals_in_their_order():
    from sklearn.gaussian_process.kernels import RationalQuadratic

    from bayesianoptimization_amd.engine import GroupEngine

    opt, eng = _optimizer()
    for bad in (0, -1, 65, 1.5, True, None):
        with pytest.raises(ValueError, match="q must be an integer in \\[1, 64\\]"):
            suggest_qnehvi(opt, bad)
    with pytest.raises(ValueError, match="n_random"):
        suggest_qnehvi(opt, 2, n_random=0)
    with pytest.raises(ValueError, match="q must not exceed n_random"):
        suggest_qnehvi(opt, 5, n_random=4)
    for bad in (0, 257, 2.5, True, None):
        with pytest.raises(ValueError, match="n_draws must be an integer in \\[1, 256\\]"):
            suggest_qnehvi(opt, 2, n_draws=bad)
    for bad in (0, 4097):
        with pytest.raises(ValueError, match="n_features must be in \\[1, 4096\\]"):
            suggest_qnehvi(opt, 2, n_features=bad)
    for bad, match in ((np.zeros((2, D + 1)), "pending must be"), (np.full((1, D), np.nan), "finite"), ([{"a": 0.5}], "lacks")):
        with pytest.raises(ValueError, match=match):
            suggest_qnehvi(opt, 2, pending=bad)
    assert not eng.calls
    # the argument checks come first: three objectives with a bad count hear about the count, then about the objectives
    three, eng3 = _optimizer(3)
    with pytest.raises(ValueError, match="n_draws"):
        suggest_qnehvi(three, 2, n_draws=0)
    with pytest.raises(NotImplementedError, match="suggest_qnehvi: 3 objectives"):
        suggest_qnehvi(three, 2)
    assert not eng3.calls
    # ... then ParetoOptimizer.suggest's refusals in its order: the empty store, the device group, the host-mode model
    group = object.__new__(GroupEngine)
    group.__dict__.update(_g=None, _h=None)
    empty, _ = _optimizer(2, n=0, engine=group, kernel=RationalQuadratic())
    with pytest.raises(A.TargetSpaceEmptyError, match="without previous samples"):
        suggest_qnehvi(empty, 2)
    opt, _ = _optimizer(2, engine=group, kernel=RationalQuadratic())
    with pytest.raises(NotImplementedError, match="suggest_qnehvi: a device group"):
        suggest_qnehvi(opt, 2)
    with pytest.raises(NotImplementedError, match="device group"):
        GroupEngine.qnehvi_greedy(group, [[], []], 1, [0.0, 0.0])
    opt, eng = _optimizer(2, kernel=RationalQuadratic())
    with pytest.raises(NotImplementedError, match="objective 0's model runs on the host"):
        suggest_qnehvi(opt, 2)
    assert not eng.calls
    # an engine without the call
    from helpers import FakeEngine

    opt, eng = _optimizer(2, engine=FakeEngine())
    with pytest.raises(NotImplementedError, match="suggest_qnehvi: the engine has no qnehvi_greedy"):
        suggest_qnehvi(opt, 2)
    # a front that outgrows the cap is NotImplementedError, as the engine raises it
    opt, eng = _optimizer()
    eng.qnehvi_greedy = lambda *a, **k: (_ for _ in ()).throw(NotImplementedError("qnehvi_greedy: the front of draw 3 outgrew 128 points"))
    with pytest.raises(NotImplementedError, match="draw 3 outgrew"):
        suggest_qnehvi(opt, 2, n_random=M, n_draws=2, n_features=8)
    # an empty pending list is no pending point
    opt, eng = _optimizer()
    suggest_qnehvi(opt, 1, n_random=M, n_draws=2, n_features=8, pending=[])
    assert np.array_equal(eng.qnehvi_args["base"], opt.params)


def test_exported_and_docstrings_point_here():
    import bayesianoptimization_amd as pkg
    from bayesianoptimization_amd import multiobjective, qnehvi

    assert "suggest_qnehvi" in pkg.__all__ and pkg.suggest_qnehvi is qnehvi.suggest_qnehvi
    for doc in (multiobjective.__doc__, ParetoOptimizer.__doc__, ParetoOptimizer.suggest.__doc__):
        assert "suggest_qnehvi" in doc


def test_header_binding_and_limits_agree():
    hdr = open(os.path.join(ROOT, "include", "gpbo.h")).read()
    assert _lib.ABI_VERSION == 4 and "#define GPBO_ABI_VERSION 4" in hdr
    assert _lib.MAX_QNEHVI_FRONT == 128 == Q.L and re.search(r"^#define GPBO_MAX_QNEHVI_FRONT 128\b", hdr, flags=re.M)
    assert _lib.MAX_QNEHVI_BASE == 16384 and re.search(r"^#define GPBO_MAX_QNEHVI_BASE  16384\b", hdr, flags=re.M)
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"^int gpbo_qnhvi_greedy\((.*?)\);", plain, flags=re.M | re.S)
    assert m, "gpbo_qnhvi_greedy is not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["gpbo_ctx* ctx", "const double* y_mean", "const double* y_std", "int n_groups", "int n_paths", "int n_features",
                    "const double* omega", "const double* phase", "const double* weights", "const double* eps", "const double* ref",
                    "const double* base", "int n_base", "int d", "int q", "int64_t index_offset", "int64_t* pick_idx",
                    "double* pick_gain", "int* front_size_out", "double* fronts_out", "double* values_out", "double* base_values_out",
                    "double* keys_out"]
    res, argtypes = _lib.SIGNATURES["gpbo_qnhvi_greedy"]
    dp, ip, np_ = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int)
    assert res is C.c_int and argtypes == [C.c_void_p, dp, dp, C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, C.c_int, C.c_int,
                                           C.c_int, C.c_int64, ip, dp, np_, dp, dp, dp, dp]
    # the debug entry points: declared in the debug part, bound, exported by the debug library only
    head, rest = plain.split("#ifdef GPBO_DEBUG", 1)
    for name in ("gpbo_debug_qnehvi_fronts", "gpbo_debug_qnehvi_stage_ms"):
        assert name in rest.split("#endif", 1)[0] and name not in head and name in _lib.DEBUG_SIGNATURES
    prod, dbg = C.CDLL(_lib.LIB_PATH), C.CDLL(_lib.DEBUG_LIB_PATH)
    assert hasattr(prod, "gpbo_qnhvi_greedy") and hasattr(dbg, "gpbo_qnhvi_greedy") and prod.gpbo_abi_version() == 4
    assert hasattr(dbg, "gpbo_debug_qnehvi_fronts") and not hasattr(prod, "gpbo_debug_qnehvi_fronts")
    # no group / communicator form
    assert not [n for n in _lib.SIGNATURES if ("qnhvi" in n or "qnehvi" in n) and n != "gpbo_qnhvi_greedy"]
