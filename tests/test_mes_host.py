"""CPU: max-value entropy search's host side — the three-range form of h (tests/mes_truth.py: `mes_values`) against the 60-digit
truth over the whole gamma range, its limits and conventions, and `suggest_mes` over an oracle-backed engine double: the engine
calls, every refusal, the RandomState it leaves behind, the floor on y*, the pick.  The device's arithmetic is checked in
tests/test_gpu_mes.py."""
import functools
import os
import re

import numpy as np
import pytest

import batch_truth as B
import mes_truth as T
import paths_ascent_truth as PA
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd import _lib, suggest_mes, suggest_thompson
from conftest import ROOT

SWITCH_POINTS = [-1e6, -1e3, -40.0, -28.0, np.nextafter(-28.0, 0.0), np.nextafter(-28.0, -40.0), -1.0, np.nextafter(-1.0, 0.0),
                 np.nextafter(-1.0, -2.0), 0.0, np.nextafter(0.0, 1.0), -np.nextafter(0.0, 1.0), 36.0]


# ---- h: the three-range form against the truth ----------------------------------------------------------------------------------
def test_three_range_form_against_the_truth():
    """A few thousand gammas over [-40, 36] plus the switch points and the far lower tail: within 1e-9 relative of the 60-digit
    truth (measured: 5.7e-14, against a (1 + gamma^2) eps model)."""
    rs = np.random.RandomState(5)
    g = np.concatenate([np.linspace(-40.0, 36.0, 3041), rs.uniform(-40.0, 36.0, 1000), rs.uniform(-2.0, 2.0, 400), SWITCH_POINTS])
    got = T.h_values(g)
    want = np.array([T.h_truth_f(v) for v in g])
    rel = np.abs(got - want) / np.abs(want)
    model = rel / ((1.0 + np.minimum(g * g, 1e6)) * np.finfo(float).eps)
    print(f"worst relative error {rel.max():.2e} at gamma = {g[rel.argmax()]!r}; worst error / ((1 + g^2) eps) = {model.max():.2f}")
    assert (want > 0).all() and rel.max() <= T.BAR
    # what the complement branch is for: log(Phi) of a Phi rounded next to 1 is 0.2 % off at gamma = 8 and 0.9 % at gamma = 15
    from scipy import special
    for gv, off in ((8.0, 1e-3), (15.0, 5e-3)):
        naive = gv * np.exp(-gv * gv / 2) / np.sqrt(2 * np.pi) / (2 * special.ndtr(gv)) - np.log(special.ndtr(gv))
        assert abs(naive - T.h_truth_f(gv)) / T.h_truth_f(gv) > off


def test_limits_and_monotonicity():
    g = np.concatenate([-np.geomspace(1e8, 1.0, 200), np.linspace(-1.0, 37.0, 2000)[1:]])
    h = T.h_values(g)
    assert (np.diff(h) < 0).all() and (h > 0).all()                           # strictly decreasing, positive while representable
    assert abs(T.h_values(np.array([0.0]))[0] - np.log(2.0)) <= 2 * np.finfo(float).eps
    assert abs(T.h_truth_f(0.0) - np.log(2.0)) <= 2 * np.finfo(float).eps
    tail = T.h_values(np.array([40.0, 41.0, 1e3, 1e300, np.inf]))
    assert (tail == 0.0).all()
    assert (np.diff(T.h_values(np.linspace(36.0, 40.0, 500))) <= 0).all()      # subnormal, then 0: still never increasing
    # the lower tail grows like log|gamma|: finite at -1e6, -1e150 and below, +inf at -inf
    low = T.h_values(np.array([-1e6, -1e150, -1e200, -1e308, -np.inf]))
    assert np.isfinite(low[:4]).all() and low[4] == np.inf and (np.diff(low) > 0).all()
    assert abs(low[0] - T.h_truth_f(-1e6)) <= T.BAR * low[0]
    assert abs(low[1] - (-0.5 + T.HALF_LOG_2PI + 150 * np.log(10.0))) <= 1e-13 * low[1]
    # the limit form meets the ratio form where it takes over
    a, b = T.h_values(np.array([-1e150, np.nextafter(-1e150, -np.inf)]))
    assert abs(a - b) <= 4 * np.finfo(float).eps * a


def test_conventions():
    mu = np.array([0.3, 0.3, np.nan, np.nan, 0.3, 0.1])
    sd = np.array([0.0, 0.2, 0.0, 0.2, np.nan, 0.0])
    a = T.mes_values(mu, sd, [0.5, 0.9])
    assert a[0] == 0.0 and a[5] == 0.0 and a[1] > 0.0 and np.isnan(a[2:5]).all()
    # the sum runs s = 0 .. S - 1, then one division: a candidate alone gives the bits it gives among others
    full = T.mes_values(np.linspace(-1, 1, 50), np.full(50, 0.3), [0.2, 0.7, 1.5])
    assert T.mes_values(np.linspace(-1, 1, 50)[17:18], [0.3], [0.2, 0.7, 1.5])[0] == full[17]
    h = T.h_values((np.array([0.2, 0.7, 1.5]) - np.linspace(-1, 1, 50)[17]) / 0.3)
    assert full[17] == ((0.0 + h[0]) + h[1] + h[2]) / 3.0


def test_one_sample_ranks_by_minus_gamma():
    rs = np.random.RandomState(2)
    mu, sd = rs.standard_normal(800), rs.uniform(0.01, 2.0, 800)
    y = 1.7
    keep = (y - mu) / sd < 36.0          # above, h is subnormal and then 0: the candidates tie
    mu, sd = mu[keep][:500], sd[keep][:500]
    g = (y - mu) / sd
    assert g.shape == (500,) and g.min() < -1.0 and g.max() > 20.0
    a = T.mes_values(mu, sd, [y])
    assert np.array_equal(np.argsort(-a, kind="stable"), np.argsort(g, kind="stable"))
    bi, bv, si, sv = T.argbest(-a, k=7, index_offset=100)
    assert bi == 100 + int(g.argmin()) and bv == -a.max() and np.array_equal(si, 100 + np.argsort(g, kind="stable")[:7])
    # argbest: the first NaN wins the arg-best and sorts last among the seeds; -0.0 ties with 0.0 to the lowest index
    bi, bv, si, sv = T.argbest(np.array([0.0, -0.0, np.nan, -1.0, np.nan]), k=5)
    assert bi == 2 and np.isnan(bv) and si.tolist() == [3, 0, 1, 2, 4]
    assert T.separated_top([3.0, 1.0, 2.0, 2.0], 1) and not T.separated_top([3.0, 1.0, 2.0, 2.0], 2)


# ---- suggest_mes over the engine double --------------------------------------------------------------------------------------------
D, N, M = 3, 30, 600
BOUNDS = B.SUGGEST_BOUNDS


class MesFakeEngine(PA.AscentFakeEngine):
    """paths_ascent_truth.AscentFakeEngine (TEST DOUBLE ONLY) + mes_argbest over `mes_values` on the resident posterior."""

    def mes_argbest(self, y_star, k_seeds=0, index_offset=0, return_values=False):
        y_star = np.atleast_1d(np.asarray(y_star, dtype=np.float64))
        self.calls.append(("mes_argbest", y_star.shape[0], k_seeds))
        self.y_star = y_star.copy()
        if not (1 <= y_star.shape[0] <= 64) or not np.isfinite(y_star).all():
            raise ValueError("mes_argbest: bad y_star")
        mu, sd = self.post[0]
        ys = -T.mes_values(mu, sd, y_star)
        bi, bv, si, sv = T.argbest(ys, k_seeds, index_offset)
        return bi, bv, si, sv, (ys if return_values else None)


_driver = functools.partial(B.suggest_driver, MesFakeEngine, n_random=M)
_same_state = B.same_state


def _floor(drv, floor_sigmas):
    gp = drv._gp
    return float(drv._space.target.max()) + floor_sigmas * np.sqrt(float(gp.alpha)) * float(gp._y_train_std)


@pytest.mark.parametrize("n_samples,refine", [(1, 2), (3, 0), (17, 1)])
def test_pick_calls_randomstate_and_info(n_samples, refine):
    n_features = 32
    drv, eng, X, y = _driver()
    twin, teng, _, _ = _driver()
    fn = drv._acquisition_function
    before = (fn.i, fn.kappa)
    Xq = BOUNDS[:, 0] + np.random.RandomState(9).uniform(size=(20, D)) * (BOUNDS[:, 1] - BOUNDS[:, 0])
    params, info = suggest_mes(drv, n_samples, n_random=M, n_features=n_features, refine=refine, floor_sigmas=0.0, return_info=True)
    suggest_thompson(twin, n_samples, n_random=M, n_features=n_features, refine=refine)
    # the RandomState ends where suggest_thompson(q = n_samples) leaves it, over the same candidates
    assert _same_state(drv._random_state, twin._random_state) and np.array_equal(eng.Xc, teng.Xc)
    # the engine calls: one fit, one candidate draw, one posterior pass, a path call per group of 16, one mes_argbest, one row fetched
    names = [c[0] for c in eng.calls]
    call = "ascend_paths" if refine else "sample_paths"
    assert names.count("fit") == 1 and names.count("generate_candidates_like") == 1 and names.count("posterior") == 1
    assert [c[2] for c in eng.calls if c[0] == call] == [16] * (n_samples // 16) + ([n_samples % 16] if n_samples % 16 else [])
    assert names.count("mes_argbest") == 1 and [c for c in eng.calls if c[0] == "mes_argbest"][0][1:] == (n_samples, 0)
    assert not {"sample_paths" if refine else "ascend_paths", "posterior_refresh", "acq_argbest", "fit_append", "polish_seeds",
                "predict_grad", "set_candidates"} & set(names)
    assert names.index("fit") < names.index("generate_candidates_like") < names.index("posterior") < names.index(call) \
        < names.index("mes_argbest")
    assert (fn.i, fn.kappa) == before                                        # the policy is neither consulted nor advanced
    # return_info: shapes, and the pick is the candidate the truth ranks first under the returned y*
    assert list(params) == drv._space.keys
    assert set(info) == {"y_star", "value", "index"} and info["y_star"].shape == (n_samples,) and np.isfinite(info["y_star"]).all()
    assert isinstance(info["index"], int) and isinstance(info["value"], float)
    assert np.array_equal(info["y_star"], eng.y_star)
    mu, sd = eng.post[0]
    a = T.mes_values(mu, sd, info["y_star"])
    assert info["index"] == int(a.argmax()) and info["value"] == a.max() and info["value"] > 0.0
    assert np.array_equal(np.array(list(params.values())), eng.Xc[info["index"]])
    # y*: with refine the best finite run of each draw, without it the draw's maximum among the candidates; never below the floor
    floor = _floor(drv, 0.0)
    assert (info["y_star"] >= floor).all()
    cand_max = np.concatenate([v.max(axis=1) for v in eng.path_values])
    assert cand_max.shape == (n_samples,)
    free = info["y_star"] > floor
    if refine:
        assert (info["y_star"][free] >= cand_max[free] - 1e-9 * max(1.0, np.abs(cand_max).max())).all()   # the climb accepts no worse point
    else:
        assert np.array_equal(info["y_star"][free], cand_max[free])
    assert np.array_equal(info["y_star"][~free], np.full((~free).sum(), floor))
    # without return_info the dict alone comes back, and equal seeds give equal answers
    again, aeng, _, _ = _driver()
    assert suggest_mes(again, n_samples, n_random=M, n_features=n_features, refine=refine, floor_sigmas=0.0) == params
    # gp.predict answers for the real data as before
    mu1, sd1 = drv._gp.predict(Xq, return_std=True)
    mu0, sd0 = twin._gp.predict(Xq, return_std=True)
    assert np.array_equal(mu0, mu1) and np.array_equal(sd0, sd1)
    assert eng.inputs[0][0].shape[0] == N and drv._gp.X_train_.shape[0] == N


def test_the_floor_is_applied():
    """A floor far above every draw's maximum replaces every y*; the default (5 noise standard deviations above the best
    observation) sits between; floor_sigmas = 0 is the best observation itself."""
    drv, eng, X, y = _driver()
    _, free = suggest_mes(drv, 5, n_random=M, n_features=32, refine=0, floor_sigmas=0.0, return_info=True)
    drv, eng, X, y = _driver()
    _, high = suggest_mes(drv, 5, n_random=M, n_features=32, refine=0, floor_sigmas=1e6, return_info=True)
    assert np.array_equal(high["y_star"], np.full(5, _floor(drv, 1e6))) and (high["y_star"] > free["y_star"].max()).all()
    drv, eng, X, y = _driver()
    _, dflt = suggest_mes(drv, 5, n_random=M, n_features=32, refine=0, return_info=True)
    assert (dflt["y_star"] >= _floor(drv, 5.0)).all() and _floor(drv, 5.0) > y.max()
    assert np.array_equal(dflt["y_star"], np.maximum(free["y_star"], _floor(drv, 5.0)))
    # a y* that is not finite takes the floor as well
    drv, eng, X, y = _driver()
    real = eng.sample_paths

    def broken(*args, **kw):
        best, val, values = real(*args, **kw)
        val = val.copy()
        val[1] = np.nan
        return best, val, values

    eng.sample_paths = broken
    _, info = suggest_mes(drv, 5, n_random=M, n_features=32, refine=0, floor_sigmas=2.0, return_info=True)
    assert info["y_star"][1] == _floor(drv, 2.0) and np.isfinite(info["y_star"]).all()


def test_refusals():
    drv, eng, X, y = _driver()
    for bad in (0, -1, 65, 1.5, True, None):
        with pytest.raises(ValueError, match="n_samples"):
            suggest_mes(drv, bad)
    for kw in ({"n_features": 0}, {"n_features": 4097}, {"n_random": 0}, {"floor_sigmas": -0.5}, {"floor_sigmas": np.nan},
               {"floor_sigmas": np.inf}, {"refine": 9}, {"refine": -1}, {"refine": 1.5}, {"refine": True}):
        with pytest.raises(ValueError):
            suggest_mes(drv, 2, **kw)
    assert not eng.calls
    group = B.check_shared_refusals(lambda d: suggest_mes(d, 2), _driver, "suggest_mes")
    with pytest.raises(NotImplementedError, match="device group"):
        type(group).mes_argbest(group, [1.0])
    # an engine without the calls
    drv, eng, X, y = _driver()
    drv._gp.engine = PA.P.PathsFakeEngine()
    with pytest.raises(NotImplementedError, match="mes_argbest"):
        suggest_mes(drv, 2)
    # any policy is fine: it is not consulted
    drv, eng, X, y = _driver(A.GPHedge([A.UpperConfidenceBound(kappa=2.0), A.ExpectedImprovement(xi=0.01)]))
    assert list(suggest_mes(drv, 2, n_random=M, n_features=16, refine=0)) == drv._space.keys


def test_exported():
    import bayesianoptimization_amd as pkg
    from bayesianoptimization_amd import mes

    assert "suggest_mes" in pkg.__all__ and pkg.suggest_mes is mes.suggest_mes


def test_header_binding_and_limits_agree():
    hdr = open(os.path.join(ROOT, "include", "gpbo.h")).read()
    assert _lib.ABI_VERSION == 4 and "#define GPBO_ABI_VERSION 4" in hdr
    assert _lib.MAX_MES_SAMPLES == 64 and re.search(r"^#define GPBO_MAX_MES_SAMPLES 64\b", hdr, flags=re.M)
    m = re.search(r"^int gpbo_mes_argbest\((.*?)\);", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), flags=re.M | re.S)
    assert m, "gpbo_mes_argbest is not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["gpbo_ctx* ctx", "int n_samples", "const double* y_star", "int k_seeds", "int64_t index_offset",
                    "int64_t* best_idx", "double* best_val", "int64_t* seed_idx", "double* seed_val", "double* ys_out"]
    import ctypes as C

    res, argtypes = _lib.SIGNATURES["gpbo_mes_argbest"]
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    assert res is C.c_int and argtypes == [C.c_void_p, C.c_int, dp, C.c_int, C.c_int64, ip, dp, ip, dp, dp]
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "gpbo_mes_argbest") and lib.gpbo_abi_version() == 4
    # no group / communicator form
    assert not [n for n in _lib.SIGNATURES if "mes" in n and n != "gpbo_mes_argbest"]
