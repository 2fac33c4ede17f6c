"""CPU: greedy batch noisy expected improvement's host side — the greedy of tests/qnei_truth.py on small hand-made values (the
conventions of include/gpbo.h), and `suggest_qnei` over an oracle-backed engine double: the order of the refusals, the engine
calls, the RandomState it leaves behind, the rounding of n_draws, `pending` in both forms, `noisy=False`, the info dict and the
zero-gain tail.  The device's arithmetic is checked in tests/test_gpu_qnei.py."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import batch_truth as B
import paths_truth as P
import qnei_truth as Q
from bayesianoptimization_amd import _lib, suggest_qnei
from bayesianoptimization_amd.qnei import draw_layout
from bayesianoptimization_amd.thompson import spectral_draw
from conftest import ROOT

D, N, M = 3, B.SUGGEST_N, 63
BOUNDS = B.SUGGEST_BOUNDS
_driver = functools.partial(B.suggest_driver, Q.QneiFakeEngine, n_random=M)


# ---- the greedy itself ------------------------------------------------------------------------------------------------------------
def test_greedy_by_hand():
    vals = np.array([[1.0, 3.0, 2.0, 0.0],
                     [2.0, 1.0, 4.0, 0.0]])
    idx, gain, keys, m = Q.greedy(vals, np.array([1.5, 1.5]), 4, index_offset=100)
    # step 0: terms (0, 1.5, .5, 0) and (.5, 0, 2.5, 0): means .25, .75, 1.5, 0 -> candidate 2; m = (2, 4)
    assert np.array_equal(keys[0], [-0.25, -0.75, -1.5, -0.0]) and idx[0] == 102 and gain[0] == 1.5
    # step 1: terms (0, 1, -, 0) and zeros: .5 at candidate 1; m = (3, 4); then nothing lifts any incumbent: the lowest unpicked index
    assert np.array_equal(keys[1], [0.0, -0.5, np.inf, 0.0]) and idx[1] == 101 and gain[1] == 0.5
    assert np.array_equal(keys[2], [0.0, np.inf, np.inf, 0.0]) and idx[2] == 100 and gain[2] == 0.0
    assert idx[3] == 103 and gain[3] == 0.0 and np.array_equal(m, [3.0, 4.0])
    assert not np.signbit(gain[2:]).any()


def test_greedy_conventions():
    nan = np.nan
    # a NaN value makes the candidate's key NaN: the first NaN wins its step with a NaN gain, leaves m as it was, and is masked
    vals = np.array([[1.0, nan, 5.0], [2.0, 0.0, nan]])
    idx, gain, keys, m = Q.greedy(vals, np.array([0.0, 0.0]), 3)
    assert idx.tolist() == [1, 2, 0] and np.isnan(gain[:2]).all() and gain[2] == 1.0      # (0 + 2) / 2 over m = (5, 0)
    assert np.isnan(keys[0][1:]).all() and keys[1][1] == np.inf and np.isnan(keys[1][2])
    assert np.array_equal(m, [5.0, 2.0])                    # fmax dropped both NaNs
    # ties go to the lowest index; the baseline: fmax in index order, NaN only when every value is
    idx, gain, _, _ = Q.greedy(np.array([[2.0, 7.0, 7.0, 1.0]]), np.array([0.0]), 2)
    assert idx.tolist() == [1, 0] and gain.tolist() == [7.0, 0.0]      # 1 before its twin 2; then nothing is left to gain: the lowest index
    assert np.array_equal(Q.baseline([[1.0, nan, 3.0], [nan, nan, nan]]), [3.0, nan], equal_nan=True)
    assert np.array_equal(Q.baseline([[1.0, 9.0]], [[0.5, 2.0]], noisy=False, y_best=1.25), [2.0])
    assert np.array_equal(Q.baseline([[1.0, 9.0]], None, noisy=False, y_best=1.25), [1.25])
    # a NaN incumbent counts as "no improvement", not as NaN
    assert np.array_equal(Q.keys_of(np.array([[1.0, 2.0]]), np.array([nan]), np.zeros(2, bool)), [-0.0, -0.0])
    # the sum runs t = 0 .. T - 1 into one accumulator, then one division
    rs = np.random.RandomState(0)
    v, m0 = rs.standard_normal((7, 5)), rs.standard_normal(7) - 1.0
    want = 0.0
    for t in range(7):
        want = want + max(v[t, 3] - m0[t], 0.0)
    assert Q.keys_of(v, m0, np.zeros(5, bool))[3] == -(want / 7.0)


def test_draw_layout_rounds_up_to_equal_groups():
    assert [draw_layout(n) for n in (1, 16, 17, 20, 32, 33, 64, 250, 256)] == \
        [(1, 1), (1, 16), (2, 9), (2, 10), (2, 16), (3, 11), (4, 16), (16, 16), (16, 16)]
    for n in range(1, 257):
        G, S = draw_layout(n)
        assert 1 <= G <= 16 and 1 <= S <= 16 and n <= G * S < n + G


# ---- suggest_qnei over the engine double ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_draws,noisy,pending_form", [(10, True, None), (20, False, "dicts"), (33, True, "array")])
def test_picks_calls_randomstate_and_info(n_draws, noisy, pending_form):
    n_features, q = 32, 4
    drv, eng, X, y = _driver()
    twin, teng, _, _ = _driver()
    pend_rows = BOUNDS[:, 0] + np.random.RandomState(4).uniform(size=(2, D)) * (BOUNDS[:, 1] - BOUNDS[:, 0])
    pending = {None: None, "array": pend_rows, "dicts": [dict(zip(drv._space.keys, r)) for r in pend_rows]}[pending_form]
    fn = drv._acquisition_function
    before = (fn.i, fn.kappa)
    picks, info = suggest_qnei(drv, q, n_random=M, n_draws=n_draws, n_features=n_features, noisy=noisy, pending=pending,
                               return_info=True)
    G, S = draw_layout(n_draws)
    # the engine calls: one fit, one candidate draw, ONE qnei_greedy call, one fetch of rows; no posterior pass, no other path call
    names = [c[0] for c in eng.calls]
    assert names.count("fit") == 1 and names.count("generate_candidates_like") == 1 and names.count("qnei_greedy") == 1
    assert [c for c in eng.calls if c[0] == "qnei_greedy"][0][1:] == (0, G, S, q)
    assert not {"sample_paths", "ascend_paths", "posterior", "posterior_refresh", "acq_argbest", "fit_append", "set_candidates"} & set(names)
    assert names.index("fit") < names.index("generate_candidates_like") < names.index("qnei_greedy")
    assert (fn.i, fn.kappa) == before
    # the RandomState: the twin's fit and candidate draw, then per group spectral_draw, (S, F) normals, (S, N) normals
    twin._gp.fit(twin._space.params, twin._space.target)
    rng, gp = twin._random_state, twin._gp
    teng.generate_candidates_like(M, BOUNDS[:, 0], BOUNDS[:, 1], rng)
    assert np.array_equal(teng.Xc, eng.Xc)
    for g in range(G):
        omega, phase = spectral_draw(gp._kind, n_features, D, rng)
        w = rng.standard_normal((S, n_features))
        eps = rng.standard_normal((S, N)) * np.sqrt(float(gp.alpha))
        got = eng.qnei_args["groups"][g]
        assert all(np.array_equal(a, b) for a, b in zip(got, (omega, phase, w, eps)))
    assert B.same_state(drv._random_state, rng)
    # what the call was given
    a = eng.qnei_args
    assert a["noisy"] is noisy and a["y_best"] == float(y.max())
    assert (a["y_mean"], a["y_std"]) == (float(drv._gp._y_train_mean), float(drv._gp._y_train_std))
    assert (a["pending"] is None) if pending is None else np.array_equal(a["pending"], pend_rows)
    # the info dict, and the picks are the greedy's on the engine's own values
    assert set(info) == {"gain", "index", "baseline", "n_draws"} and info["n_draws"] == G * S >= n_draws
    assert info["gain"].shape == (q,) and info["index"].shape == (q,) and info["baseline"].shape == (G * S,)
    idx, gain, _, _ = Q.greedy(eng.qnei_values, eng.qnei_baseline, q)
    assert np.array_equal(info["index"], idx) and np.array_equal(info["gain"], gain) and np.array_equal(info["baseline"], eng.qnei_baseline)
    assert len(picks) == q and all(list(p) == drv._space.keys for p in picks)
    assert np.array_equal(np.array([list(p.values()) for p in picks]), eng.Xc[idx])
    assert gain[0] > 0.0 and (np.diff(gain) <= 0.0).all()                    # the gains of a greedy on a submodular score never rise
    if not noisy and pending is None:
        assert np.array_equal(info["baseline"], np.full(G * S, y.max()))
    if noisy:
        assert info["baseline"].std() > 0.0                                   # every draw has an incumbent of its own
    # without return_info the list alone comes back, and equal seeds give equal answers
    again, _, _, _ = _driver()
    assert suggest_qnei(again, q, n_random=M, n_draws=n_draws, n_features=n_features, noisy=noisy, pending=pending) == picks
    # gp.predict answers for the real data as before
    Xq = BOUNDS[:, 0] + np.random.RandomState(9).uniform(size=(20, D)) * (BOUNDS[:, 1] - BOUNDS[:, 0])
    mu1, sd1 = drv._gp.predict(Xq, return_std=True)
    mu0, sd0 = twin._gp.predict(Xq, return_std=True)
    assert np.array_equal(mu0, mu1) and np.array_equal(sd0, sd1)
    assert eng.inputs[0][0].shape[0] == N and drv._gp.X_train_.shape[0] == N


def test_pending_lowers_the_gains():
    """A pending point ON the first pick absorbs that pick's improvement: the greedy then starts where it would have gone on."""
    drv, eng, X, y = _driver()
    picks, free = suggest_qnei(drv, 3, n_random=M, n_draws=10, n_features=32, return_info=True)
    drv, eng, X, y = _driver()
    _, held = suggest_qnei(drv, 2, n_random=M, n_draws=10, n_features=32, pending=[picks[0]], return_info=True)
    # (the draws' values at the point alone and among the candidates may differ in the last bits — two matrix products —, so a gain
    # that is exactly 0 after the pick may be a few ulps after the pending point: the gains are compared, and the first index)
    assert held["index"][0] == free["index"][1] and np.allclose(held["gain"], free["gain"][1:], rtol=1e-9, atol=1e-12)
    assert (held["baseline"] >= free["baseline"]).all() and (held["baseline"] > free["baseline"]).any()


def test_zero_gain_tail():
    """q = M: every candidate exactly once; the gain reaches exactly 0 (M = 63, T = 10: at the third pick) and from there the picks
    are the unpicked indices in ascending order."""
    drv, eng, X, y = _driver()
    picks, info = suggest_qnei(drv, M, n_random=M, n_draws=10, n_features=32, return_info=True)
    idx, gain = info["index"], info["gain"]
    assert sorted(idx.tolist()) == list(range(M)) and len(picks) == M
    first_zero = int(np.argmax(gain == 0.0))
    print(f"gains {gain[:first_zero + 1].tolist()}: zero from pick {first_zero}")
    assert first_zero == 2 and (gain[:first_zero] > 0.0).all() and (gain[first_zero:] == 0.0).all()
    assert (np.diff(idx[first_zero:]) > 0).all()
    # every draw's maximum among the candidates has been absorbed by then
    m = np.fmax.reduce(np.column_stack([info["baseline"]] + [eng.qnei_values[:, i] for i in idx[:first_zero]]), axis=1)
    assert (m >= eng.qnei_values.max(axis=1)).all()


def test_refusals_in_their_order():
    drv, eng, X, y = _driver()
    for bad in (0, -1, 65, 1.5, True, None):
        with pytest.raises(ValueError, match="q must be an integer in \\[1, 64\\]"):
            suggest_qnei(drv, bad)
    with pytest.raises(ValueError, match="n_random"):
        suggest_qnei(drv, 2, n_random=0)
    with pytest.raises(ValueError, match="q must not exceed n_random"):
        suggest_qnei(drv, 5, n_random=4)
    for bad in (0, 257, 2.5, True, None):
        with pytest.raises(ValueError, match="n_draws must be an integer in \\[1, 256\\]"):
            suggest_qnei(drv, 2, n_draws=bad)
    for bad in (0, 4097):
        with pytest.raises(ValueError, match="n_features must be in \\[1, 4096\\]"):
            suggest_qnei(drv, 2, n_features=bad)
    with pytest.raises(ValueError, match="at most 64"):
        suggest_qnei(drv, 2, pending=np.zeros((65, D)))
    assert not eng.calls
    # the argument checks come first, then the gate: an un-accelerated optimizer with a bad count hears about the count
    drv._gp = object()
    with pytest.raises(ValueError, match="n_draws"):
        suggest_qnei(drv, 2, n_draws=0)
    with pytest.raises(NotImplementedError, match="suggest_qnei: .*accelerate"):
        suggest_qnei(drv, 2, pending=np.zeros((2, D + 1)))           # ... and the gate comes before what needs the space
    group = B.check_shared_refusals(lambda d: suggest_qnei(d, 2), _driver, "suggest_qnei")
    with pytest.raises(NotImplementedError, match="device group"):
        type(group).qnei_greedy(group, [], 1)
    # pending of another shape, not finite, or lacking a parameter: after the gate, before anything runs
    for bad, match in ((np.zeros((2, D + 1)), "pending must be"), (np.full((1, D), np.nan), "finite"), ([{"x0": 0.5}], "lacks")):
        drv, eng, X, y = _driver()
        with pytest.raises(ValueError, match=match):
            suggest_qnei(drv, 2, pending=bad)
        assert not eng.calls
    # an engine without the call
    drv, eng, X, y = _driver()
    drv._gp.engine = P.PathsFakeEngine()
    with pytest.raises(NotImplementedError, match="suggest_qnei: the engine has no sample_paths / qnei_greedy"):
        suggest_qnei(drv, 2)
    # an empty pending list is no pending point
    drv, eng, X, y = _driver()
    suggest_qnei(drv, 1, n_random=M, n_draws=2, n_features=8, pending=[])
    assert eng.qnei_args["pending"] is None


def test_exported():
    import bayesianoptimization_amd as pkg
    from bayesianoptimization_amd import qnei

    assert "suggest_qnei" in pkg.__all__ and pkg.suggest_qnei is qnei.suggest_qnei


def test_header_binding_and_limits_agree():
    hdr = open(os.path.join(ROOT, "include", "gpbo.h")).read()
    assert _lib.ABI_VERSION == 4 and "#define GPBO_ABI_VERSION 4" in hdr
    assert _lib.MAX_QNEI_GROUPS == 16 and re.search(r"^#define GPBO_MAX_QNEI_GROUPS 16\b", hdr, flags=re.M)
    assert _lib.MAX_QNEI_POINTS == 64 and re.search(r"^#define GPBO_MAX_QNEI_POINTS 64\b", hdr, flags=re.M)
    assert _lib.MAX_SEEDS == 64 and _lib.MAX_PATHS == 16
    m = re.search(r"^int gpbo_qnei_greedy\((.*?)\);", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), flags=re.M | re.S)
    assert m, "gpbo_qnei_greedy is not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["gpbo_ctx* ctx", "int slot", "double y_mean", "double y_std", "int n_groups", "int n_paths", "int n_features",
                    "const double* omega", "const double* phase", "const double* weights", "const double* eps", "int noisy",
                    "double y_best", "const double* pending", "int n_pending", "int d", "int q", "int64_t index_offset",
                    "int64_t* pick_idx", "double* pick_gain", "double* baseline_out", "double* values_out", "double* keys_out"]
    res, argtypes = _lib.SIGNATURES["gpbo_qnei_greedy"]
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    assert res is C.c_int and argtypes == [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, dp, dp, dp, dp,
                                           C.c_int, C.c_double, dp, C.c_int, C.c_int, C.c_int, C.c_int64, ip, dp, dp, dp, dp]
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        lib = C.CDLL(path)
        assert hasattr(lib, "gpbo_qnei_greedy") and lib.gpbo_abi_version() == 4
    # no group / communicator form
    assert not [n for n in _lib.SIGNATURES if "qnei" in n and n != "gpbo_qnei_greedy"]
