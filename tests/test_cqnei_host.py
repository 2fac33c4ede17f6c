"""CPU: suggest_constrained_qnei against a test double (tests/cnei_truth.py: CneiFakeEngine) — the order of its checks and their
exception types, the RandomState draws in the documented order (replayed on a twin), the floor default, the pending forms, the
export; the header's argument list against the ctypes prototype and the naming rules of the new symbols; the rule on hand-made
arrays; and, on the TRUTH alone, the conditions the GPU cases of tests/test_gpu_cnei.py rest on."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

import batch_truth as B
import cnei_truth as CT
import qnei_truth as Q
import test_scbo_host as SH
from bayesianoptimization_amd import _lib, cqnei, suggest_constrained_qnei
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd.engine import GpEngine, GroupEngine
from bayesianoptimization_amd.qnei import draw_layout
from bayesianoptimization_amd.thompson import spectral_draw
from conftest import ROOT

INF = np.inf
M, D, N = SH.M, SH.D, SH.N


def driver(**kw):
    return SH.constrained_driver(CT.CneiFakeEngine, **kw)


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
def test_rule_on_hand_made_arrays():
    nan = np.nan
    f = np.array([[1.0, 5.0, 3.0, 4.0], [2.0, 2.0, nan, 6.0]])
    c = np.array([[0.0, 2.0, 0.5, 1.0], [0.0, 0.0, 0.0, nan]])
    fb = np.array([[2.5, 9.0], [1.0, 1.5]])
    cb = np.array([[0.0, 3.0], [4.0, nan]])
    lb, ub, y_std = np.array([-INF]), np.array([1.0]), np.array([7.0, 2.0])
    t = CT.rule(np.array([f, c]), np.array([fb, cb]), lb, ub, y_std, 0.5, 3, index_offset=10)
    assert t["viol"].tolist()[0] == [0.0, 0.5, 0.0, 0.0] and np.isnan(t["viol"][1, 3])
    # the masked values: -inf where the constraint is violated, NaN where the objective or the constraint is NaN
    assert t["masked"][0].tolist() == [1.0, -INF, 3.0, 4.0] and t["masked"][1, :2].tolist() == [2.0, 2.0] and np.isnan(t["masked"][1, 2:]).all()
    # draw 0: base point 0 is feasible (2.5), point 1 is not (9.0 does not count); draw 1: nothing feasible, a NaN dropped -> the floor
    assert t["baseline"].tolist() == [2.5, 0.5]
    # step 0: candidates 2 and 3 are NaN in draw 1 -> the first NaN wins with a NaN gain and a NaN share; it lifts draw 0 to 3.0
    assert t["index"].tolist() == [12, 13, 10] and np.isnan(t["gain"][:2]).all() and np.isnan(t["feasible"][:2]).all()
    # step 2: candidate 0 (1.0 | 2.0) against (4.0, 0.5) beats the infeasible candidate 1 (-inf | 2.0) by the lower index at equal gain
    assert t["gain"][2] == (0.0 + 1.5) / 2.0 and t["feasible"][2] == 1.0 and t["final"].tolist() == [4.0, 2.0]
    assert t["keys"][2].tolist() == [-0.75, -0.75, INF, INF]
    # no base point: every draw starts from the floor
    assert CT.rule(np.array([f, c]), None, lb, ub, y_std, -1.0, 1)["baseline"].tolist() == [-1.0, -1.0]
    # every bound infinite: qnei_truth's greedy on the raw values
    t = CT.rule(np.array([f[:1], c[:1]]), None, np.array([-INF]), np.array([INF]), y_std, 0.0, 2)
    i2, g2, k2, _ = Q.greedy(f[:1], np.array([0.0]), 2)
    assert np.array_equal(t["index"], i2) and np.array_equal(t["gain"], g2) and np.array_equal(t["keys"], k2) and (t["feasible"] == 1.0).all()


# ---- suggest_constrained_qnei --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_constraints,n_draws", [(1, 5), (2, 20)])
def test_draws_one_call_and_picks(n_constraints, n_draws):
    FEATURES, q = 48, 3
    lb, ub = ((-INF,), (0.5,)) if n_constraints == 1 else ((-INF, -1.0), (0.5, 1.5))
    drv, eng, X, y, c = driver(lb=lb, ub=ub)
    twin, teng, _, _, _ = driver(lb=lb, ub=ub)
    pending = [{"x0": 0.25, "x1": 0.5, "x2": 0.75}] if n_constraints == 1 else np.array([[0.25, 0.5, 0.75], [0.5, 0.5, 1.0]])
    picks, info = suggest_constrained_qnei(drv, q, n_random=M, n_draws=n_draws, n_features=FEATURES, pending=pending, return_info=True)
    assert len(picks) == q and list(picks[0]) == drv._space.keys and drv._acquisition_function.i == 0
    # the replay: the fits (theta searches included), the candidates, then per group and within it per slot the documented draws
    rng = twin._random_state
    gps = [twin._gp, *twin._space.constraint.model]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        twin._gp.fit(twin._space.params, twin._space.target)
        twin._space.constraint.fit(twin._space.params, twin._space._constraint_values)
    teng.generate_candidates_like(M, B.SUGGEST_BOUNDS[:, 0], B.SUGGEST_BOUNDS[:, 1], rng)
    assert np.array_equal(teng.Xc, eng.Xc)
    G, S = draw_layout(n_draws)
    draws = [[] for _ in gps]
    for _ in range(G):
        for j, g in enumerate(gps):
            omega, phase = spectral_draw(g._kind, FEATURES, D, rng)
            w = rng.standard_normal((S, FEATURES))
            draws[j].append((omega, phase, w, rng.standard_normal((S, N)) * np.sqrt(float(g.alpha))))
    assert B.same_state(drv._random_state, rng)
    got = eng.cnei_args
    assert len(got["draws"]) == 1 + n_constraints and all(len(groups) == G for groups in got["draws"])
    for a, b in zip(got["draws"], draws):
        for u, v in zip(a, b):
            assert all(np.array_equal(x, z) for x, z in zip(u, v))
    assert np.array_equal(got["lb"], lb) and np.array_equal(got["ub"], ub)
    assert got["y_mean"].tolist() == [float(g._y_train_mean) for g in gps] and got["y_std"].tolist() == [float(g._y_train_std) for g in gps]
    rows = np.array([[0.25, 0.5, 0.75]]) if n_constraints == 1 else pending
    assert np.array_equal(got["base"], np.vstack([X, rows])) and got["y_floor"] == y.min() - np.ptp(y)
    # the picks are the rule's on the double's own values
    t = CT.rule(eng.cnei_values, eng.cnei_base_values, np.array(lb), np.array(ub), got["y_std"], got["y_floor"], q)
    assert B.rows_to_indices(picks, eng.Xc).tolist() == t["index"].tolist() and info["n_draws"] == G * S
    assert np.array_equal(info["index"], t["index"]) and np.array_equal(info["gain"], t["gain"], equal_nan=True)
    assert np.array_equal(info["feasible"], t["feasible"], equal_nan=True) and np.array_equal(info["baseline"], t["baseline"])
    assert set(info) == {"gain", "index", "feasible", "baseline", "n_draws"}
    names = [k[0] for k in eng.calls]
    assert names.count("fit") == 1 + n_constraints and names.count("generate_candidates_like") == 1 and names.count("cnei_greedy") == 1
    assert not {"posterior", "set_candidates", "sample_paths", "sample_paths_constrained", "qnei_greedy", "acq_argbest"} & set(names)
    assert max(i for i, k in enumerate(names) if k == "fit") < names.index("generate_candidates_like") < names.index("cnei_greedy")
    # afterwards the models answer for the real data as before
    assert np.array_equal(drv._gp.predict(X[:4]), twin._gp.predict(X[:4]))
    assert np.array_equal(drv._space.constraint.predict(X[:4]), twin._space.constraint.predict(X[:4]))


def test_floor_default_and_given():
    assert cqnei.default_floor([1.0, 3.0, 2.0]) == 1.0 - 2.0 and cqnei.default_floor([2.5, 2.5]) == 1.5 and cqnei.default_floor([4.0]) == 3.0
    drv, eng, X, y, c = driver()
    suggest_constrained_qnei(drv, 1, n_random=M, n_draws=2, n_features=8, floor=-7.25)
    assert eng.cnei_args["y_floor"] == -7.25 and np.array_equal(eng.cnei_args["base"], X)      # no pending: the observed points alone
    drv, eng, X, y, c = driver()
    suggest_constrained_qnei(drv, 1, n_random=M, n_draws=2, n_features=8, pending=[])          # an empty list is no pending point
    assert np.array_equal(eng.cnei_args["base"], X)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="floor must be finite"):
            suggest_constrained_qnei(drv, 1, floor=bad)


def test_refusals_in_their_order():
    drv, eng, X, y, c = driver()
    for bad in (0, -1, 65, 1.5, True, None):
        with pytest.raises(ValueError, match="q must be an integer in \\[1, 64\\]"):
            suggest_constrained_qnei(drv, bad)
    with pytest.raises(ValueError, match="n_random"):
        suggest_constrained_qnei(drv, 2, n_random=0)
    with pytest.raises(ValueError, match="q must not exceed n_random"):
        suggest_constrained_qnei(drv, 5, n_random=4)
    for bad in (0, 257, 2.5, True, None):
        with pytest.raises(ValueError, match="n_draws must be an integer in \\[1, 256\\]"):
            suggest_constrained_qnei(drv, 2, n_draws=bad)
    for bad in (0, 4097):
        with pytest.raises(ValueError, match="n_features must be in \\[1, 4096\\]"):
            suggest_constrained_qnei(drv, 2, n_features=bad)
    assert not eng.calls
    # the argument checks come first, then the gate: an un-accelerated optimizer with a bad count hears about the count
    drv._gp = object()
    with pytest.raises(ValueError, match="n_draws"):
        suggest_constrained_qnei(drv, 2, n_draws=0)
    with pytest.raises(NotImplementedError, match="suggest_constrained_qnei: .*accelerate"):
        suggest_constrained_qnei(drv, 2, pending=np.zeros((2, D + 1)))      # ... and the gate comes before what needs the space
    # the gate's refusals, and what can be wrong with the constraint model: the exception, its text, no engine call, no draw
    who = "suggest_constrained_qnei"
    table = [(spoil, kw, error, match.replace("suggest_turbo", "suggest_qnei")) for spoil, kw, error, match in SH._spoil_table(who)]
    assert any("use suggest_qnei" in row[3] for row in table)
    for spoil, kw, error, match in table:
        drv, eng, X, y, c = driver(**kw)
        before = drv._random_state.get_state()
        spoil(drv, eng)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with pytest.raises(error, match=match):
                suggest_constrained_qnei(drv, 2)
        assert not eng.calls, (getattr(spoil, "__name__", "host_kernel"), eng.calls)
        after = drv._random_state.get_state()
        assert np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    with pytest.raises(NotImplementedError, match="device group has no constrained batch"):
        GroupEngine.cnei_greedy(object.__new__(GroupEngine), [], 1, [], [], 0.0)
    # pending of another shape, not finite, or lacking a parameter: after the gate, before anything runs
    for bad, match in ((np.zeros((2, D + 1)), "pending must be"), (np.full((1, D), np.nan), "finite"), ([{"x0": 0.5}], "lacks")):
        drv, eng, X, y, c = driver()
        with pytest.raises(ValueError, match=match):
            suggest_constrained_qnei(drv, 2, pending=bad)
        assert not eng.calls
    # an engine without the call
    import scbo_truth as ST

    drv, eng, X, y, c = SH.constrained_driver(ST.ScboFakeEngine)
    with pytest.raises(NotImplementedError, match="suggest_constrained_qnei: the engine has no cnei_greedy"):
        suggest_constrained_qnei(drv, 2)
    assert not eng.calls
    # suggest_qnei still refuses a constraint
    from bayesianoptimization_amd import suggest_qnei

    drv, eng, X, y, c = driver()
    with pytest.raises(A.ConstraintNotSupportedError):
        suggest_qnei(drv, 2)


def test_engine_method_checks_its_shapes_on_the_host():
    eng = object.__new__(GpEngine)
    eng.__dict__.update(_n_obs={0: (4, 2), 1: (3, 2)}, _pending={}, _h=None)
    eng._settle = lambda slot: None
    t0 = (np.zeros((5, 2)), np.zeros(5), np.zeros((2, 5)), np.zeros((2, 4)))
    t1 = (np.zeros((5, 2)), np.zeros(5), np.zeros((2, 5)), np.zeros((2, 3)))
    for draws, kw, match in (([[t0]], {}, "1 \\+ C lists"), ([[t0]] * 9, {}, "n_constraints"), ([[t0], []], {}, "same non-empty list"),
                             ([[t0] * 17, [t1] * 17], {}, "n_groups"), ([[t0], [t1]], {"lb": [0.0, 0.0]}, "lb / ub"),
                             ([[t0], [t1]], {"y_std": [1.0]}, "lb / ub"), ([[t0], [t0]], {}, "do not fit the slot's model"),
                             ([[t0], [(t1[0], t1[1], t1[2][:1], t1[3][:1])]], {}, "same S and F"),
                             ([[t0], [t1]], {"base": np.zeros(3)}, "two-dimensional"), ([[t0], [t1]], {"base": np.zeros((1, 3))}, "does not fit")):
        args = {"lb": [0.0], "ub": [1.0], "y_floor": 0.0, **kw}
        with pytest.raises(ValueError, match=match):
            eng.cnei_greedy(draws, 1, args.pop("lb"), args.pop("ub"), args.pop("y_floor"), **args)


def test_exported():
    import bayesianoptimization_amd as pkg

    assert "suggest_constrained_qnei" in pkg.__all__ and pkg.suggest_constrained_qnei is cqnei.suggest_constrained_qnei


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_header_binding_names_and_limits_agree():
    hdr = open(os.path.join(ROOT, "include", "gpbo.h")).read()
    assert _lib.ABI_VERSION == 4 and "#define GPBO_ABI_VERSION 4" in hdr
    assert _lib.MAX_CNEI_BASE == 16384 and re.search(r"^#define GPBO_MAX_CNEI_BASE 16384\b", hdr, flags=re.M)
    # the product symbol and its limit are declared BEHIND the debug block, the stage timer inside it
    head, _, tail = hdr.partition("#endif /* GPBO_DEBUG */")
    assert "gpbo_cnei_greedy(" in tail and "GPBO_MAX_CNEI_BASE 16384" in tail and "int gpbo_cnei_greedy(" not in head
    debug = head.partition("#ifdef GPBO_DEBUG")[2]
    assert "int gpbo_debug_cnei_stage_ms(" in debug
    m = re.search(r"^int gpbo_cnei_greedy\((.*?)\);", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), flags=re.M | re.S)
    assert m, "gpbo_cnei_greedy is not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["gpbo_ctx* ctx", "int n_constraints", "const double* y_mean", "const double* y_std", "const double* lb",
                    "const double* ub", "int n_groups", "int n_paths", "int n_features", "const double* omega", "const double* phase",
                    "const double* weights", "const double* eps", "double y_floor", "const double* base", "int n_base", "int d", "int q",
                    "int64_t index_offset", "int64_t* pick_idx", "double* pick_gain", "double* pick_feasible", "double* baseline_out",
                    "double* values_out", "double* viol_out", "double* base_values_out", "double* keys_out"]
    res, argtypes = _lib.SIGNATURES["gpbo_cnei_greedy"]
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    kinds = {"gpbo_ctx*": C.c_void_p, "int": C.c_int, "double": C.c_double, "int64_t": C.c_int64, "const double*": dp, "double*": dp,
             "int64_t*": ip}
    assert res is C.c_int and argtypes == [kinds[a.rsplit(" ", 1)[0]] for a in args]
    assert _lib.DEBUG_SIGNATURES["gpbo_debug_cnei_stage_ms"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_float)])
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        lib = C.CDLL(path)
        assert hasattr(lib, "gpbo_cnei_greedy") and lib.gpbo_abi_version() == 4
    assert not hasattr(C.CDLL(_lib.LIB_PATH), "gpbo_debug_cnei_stage_ms")
    # the naming rules: the new names contain none of the words the siblings' host tests reserve, and there is no group /
    # communicator form
    new = [n for n in list(_lib.SIGNATURES) + list(_lib.DEBUG_SIGNATURES) if "cnei" in n]
    assert sorted(new) == ["gpbo_cnei_greedy", "gpbo_debug_cnei_stage_ms"]
    for name in new:
        assert not [w for w in ("qnei", "qnhvi", "qnehvi", "ehvi", "kg", "mes", "constrained", "trust_region") if w in name], name


# ---- the GPU cases' conditions, on the truth alone ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CT.CASES))
def test_the_gpu_cases_conditions_hold_on_the_truth(name):
    c = CT.case_of(name)
    q = min(8, c.M)
    t = c.truth(q)
    g = np.hstack([t["masked"], t["masked_base"]])
    share = float(np.mean(t["masked"] > -INF))
    near = float(c.near_a_bound().mean())
    print(f"{c.what}: feasible share {share:.3f}, pairs next to a bound {near:.2e}, bars {['%.1e' % b for b in c.bars]}")
    assert np.isfinite(g[g > -INF]).all() and not np.isnan(g).any()
    if c.share is not None:
        assert c.share[0] <= share <= c.share[1], f"{c.what}: the feasible share {share:.3f} decides too little: pick other quantiles"
    # at most 1 % of the (draw, point) pairs may be left out of the feasibility comparison (a cap, not a measurement: with bars near
    # 1e-9 the truth sits orders of magnitude inside it)
    assert near <= 0.01, f"{c.what}: {near:.2%} of the pairs are next to a bound: pick another seed"
    assert all(b < 1e-6 for b in c.bars)
    if name == CT.FLOOR_CASE:
        none = ~(t["masked_base"] > -INF).any(axis=1)
        assert none.any() and not none.all(), "the floor case needs a draw without a feasible base point and one with"
        assert np.array_equal(t["baseline"][none], np.full(none.sum(), c.y_floor)) and (t["baseline"][~none] > c.y_floor).any()
        assert 0.0 < share < 0.2
    if c.B == 0:
        assert np.array_equal(t["baseline"], np.full(c.T, c.y_floor))
    if c.picks:
        n, gaps = Q.leading_separated_steps(np.where(np.isfinite(t["masked"]), t["masked"], np.nan), t["keys"], B.GAP_FLOOR)
        assert n >= 2, f"{c.what}: only {n} separated leading steps in the truth itself: pick another seed"


def test_the_case_list_covers_the_edges():
    cases = {k: CT.Case(**v) for k, v in CT.CASES.items() if v["M"] < 1 << 17}
    assert any(c.M % 2 == 1 for c in cases.values()) and any(c.M % 2 == 0 and c.M > 512 for c in cases.values())
    assert any(c.C == 7 and c.T == 1 and c.B == 0 for c in cases.values()) and any(c.T == 256 for c in cases.values())
    assert any(CT.CASES[k]["M"] >= 1 << 17 for k in CT.CASES) and any(v.get("f32_slot") == 0 for v in CT.CASES.values())
    assert any(v.get("scaled_slot") for v in CT.CASES.values()) and CT.FLOOR_CASE in CT.CASES and len(CT.PICK_CASES) >= 2
    big = cases["c2-n130,65,64-m514-f65-d5-3x16-b194"]
    assert len(set(big.kinds)) == 3 and len(set(big.Ns)) == 3
