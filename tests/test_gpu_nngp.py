"""GPU (-m gpu): gpnn_acq_argbest — nearest-neighbour GP scoring of the resident candidates — against nngp_truth (X, y, theta and the
candidates alone); exact duplicate rows; bits alone and among 257; the selection; the refusals in the header's order; suggest_local.
Bars: the neighbour indices exactly — tests/test_nngp_host.py holds every case's k-th / (k + 1)-th d2 at least 1e-9 apart, relative,
so the device's fma and the reference's multiply-add cannot order them differently —; mu, sd and ys within max(1e-9, 4 D) (1 +
|truth|), D the reference's own fp64-versus-longdouble spread on the case (at most 2.5e-10 there, with alpha >= 1e-4)."""
import functools

import numpy as np
import pytest

import batch_truth as B
import matern_family_truth as F
import nngp_truth as T
from bayesianoptimization_amd import _lib, suggest_local
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd._lib import dptr, iptr
from bayesianoptimization_amd.engine import GroupEngine

pytestmark = pytest.mark.gpu

Y_MEAN, Y_STD, ALPHA, SCALED = 3.5, 0.4, 1e-3, (2.3, 0.05)
#        k,  N,    M,   d,  kind,       acq,     (c, w)
CASES = [(16, 16, 1, 1, F.RBF, T.UCB, None), (16, 17, 65, 3, F.MATERN25, T.EI, None), (16, 257, 257, 16, F.MATERN15, T.POI, None),
         (16, 1031, 65, 64, F.MATERN05, T.LOG_EI, None), (16, 16, 257, 16, F.MATERN25, T.UCB, None), (16, 1031, 257, 3, F.RBF, T.EI, None),
         (16, 257, 1, 64, F.MATERN15, T.UCB, None), (16, 17, 65, 1, F.MATERN05, T.POI, None), (16, 1031, 65, 16, F.MATERN25, T.UCB, SCALED),
         (32, 32, 65, 3, F.MATERN15, T.UCB, None), (32, 33, 257, 16, F.RBF, T.EI, None), (32, 257, 1, 1, F.MATERN25, T.POI, None),
         (32, 1031, 257, 64, F.MATERN25, T.UCB, None), (32, 32, 1, 64, F.MATERN05, T.EI, None), (32, 257, 65, 3, F.RBF, T.LOG_EI, None),
         (32, 1031, 65, 1, F.MATERN15, T.UCB, None), (32, 33, 65, 16, F.MATERN05, T.UCB, SCALED), (32, 1031, 257, 16, F.MATERN25, T.EI, None),
         (64, 64, 257, 3, F.MATERN25, T.UCB, None), (64, 65, 65, 16, F.MATERN15, T.EI, None), (64, 257, 257, 1, F.RBF, T.UCB, None),
         (64, 1031, 65, 3, F.MATERN05, T.POI, None), (64, 64, 65, 64, F.RBF, T.UCB, None), (64, 1031, 257, 16, F.MATERN25, T.UCB, None),
         (64, 257, 65, 64, F.MATERN15, T.LOG_EI, None), (64, 65, 1, 3, F.MATERN25, T.EI, SCALED), (64, 1031, 1, 16, F.RBF, T.UCB, None)]
IDS = ["k{}-N{}-M{}-d{}-kind{}-acq{}{}".format(*c[:6], "-scaled" if c[6] else "") for c in CASES]


def inputs(k, N, M, d, kind, acq, scaled):
    """The case's data: uniform points, length scales that leave a candidate correlated with its neighbours, an incumbent in range"""
    X, y = F.data(N, d, seed=7 * N + d + k)
    yn = (y - y.mean()) / y.std()
    ls = (0.35 if d > 1 else 0.05) * np.sqrt(d) * np.geomspace(0.75, 1.33, d)
    Xc = np.random.RandomState(300 + N + d + k).uniform(size=(M, d))
    c, w = scaled or (1.0, 0.0)
    return X, yn, ls, Xc, c, w, (2.576 if acq == T.UCB else 0.01), Y_MEAN + 0.5 * Y_STD


@functools.lru_cache(maxsize=None)
def truth(case):
    X, yn, ls, Xc, c, w, param, y_max = inputs(*case)
    return T.nngp(case[4], X, yn, ls, ALPHA, Xc, case[0], case[5], param, y_max, Y_MEAN, Y_STD, c, w)


def run(eng, case, Xc=None, X=None, k_seeds=0):
    X0, yn, ls, Xc0, c, w, param, y_max = inputs(*case)
    eng.set_candidates(Xc0 if Xc is None else Xc)
    return eng.nn_acq_argbest(X0 if X is None else X, yn, case[4], ls, ALPHA, case[0], case[5], param, y_max, amplitude=c, white=w,
                              k_seeds=k_seeds, y_mean=Y_MEAN, y_std=Y_STD, return_values=True, return_posterior=True,
                              return_neighbors=True)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_values_against_the_truth(engine, case):
    want = truth(case)
    assert want["gap"] >= 1e-9
    _bi, _bv, _si, _sv, ys, mu, sd, nbr = run(engine, case)
    assert np.array_equal(nbr, want["nbr"])
    err = [float((np.abs(g - want[n]) / (1 + np.abs(want[n]))).max()) for n, g in (("mu", mu), ("sd", sd), ("ys", ys))]
    print(f"{case}: worst error mu {err[0]:.2e}, sd {err[1]:.2e}, ys {err[2]:.2e}; D {want['D']:.2e}; gap {want['gap']:.2e}")
    assert max(err) <= max(1e-9, 4 * want["D"])
    if case[1] == case[0]:      # every row a neighbour: the exact GP, the engine's own
        X, yn, ls = inputs(*case)[:3]
        engine.fit(X, yn, case[4], ls, ALPHA)
        mu_x, sd_x = engine.posterior(0, Y_MEAN, Y_STD)
        assert np.abs(mu - mu_x).max() <= 1e-9 * (1 + np.abs(mu_x).max()) and np.abs(sd - sd_x).max() <= 1e-9 * (1 + np.abs(sd_x).max())


def test_exact_ties_go_to_the_lower_index(engine):
    case = (16, 257, 257, 3, F.MATERN25, T.UCB, None)
    X, yn, ls, Xc = inputs(*case)[:4]
    X = X.copy()
    X[100:200] = X[:100]      # a hundred exact duplicates: bit-exact ties in d2, inside the lists and at their ends
    want, _gap = T.neighbours(X, ls, Xc, 16)
    nbr = run(engine, case, X=X)[7]
    twins = ((want[:, :-1] + 100 == want[:, 1:]) & (want[:, :-1] < 100)).sum()
    assert twins > 257 and np.array_equal(nbr, want)


def test_a_candidates_bits_alone_and_among_257(engine):
    case = CASES[17]
    Xc = inputs(*case)[3]
    among = run(engine, case)[4:7]
    for i in (0, 100, 256):
        alone = run(engine, case, Xc[i:i + 1])[4:7]
        assert all(a[0] == b[i] for a, b in zip(alone, among))


@pytest.mark.parametrize("acq", [T.UCB, T.EI, T.POI, T.LOG_EI])
def test_selection_is_numpys(engine, acq):
    case = (16, 257, 257, 3, F.RBF, acq, None)
    bi, bv, si, sv, ys = run(engine, case, k_seeds=5)[:5]
    order = np.argsort(ys, kind="stable")[:5]
    assert bi == order[0] and bv == ys[order[0]] and np.array_equal(si, order) and np.array_equal(sv, ys[order])
    Xc = inputs(*case)[3].copy()
    Xc[[40, 11], [1, 0]] = np.nan      # the first NaN wins; its neighbour row says so
    bi, bv, si, _sv, ys, mu, sd, nbr = run(engine, case, Xc, k_seeds=5)
    assert bi == 11 and np.isnan(bv) and np.isnan(ys[[11, 40]]).all() and np.isfinite(np.delete(ys, [11, 40])).all()
    assert (nbr[[11, 40]] == -1).all() and np.isnan(mu[11]) and np.isnan(sd[40]) and not np.isin([11, 40], si).any()


# the header's order: each call is wrong in ITS argument and in every argument a LATER entry names, and still fails as itself
ORDER = [("k", 17, _lib.ERR_INVALID), ("N", 15, _lib.ERR_INVALID), ("d", 65, _lib.ERR_INVALID), ("n_ls", 2, _lib.ERR_INVALID),
         ("kernel", 9, _lib.ERR_UNSUPPORTED), ("acq", 4, _lib.ERR_UNSUPPORTED), ("X", None, _lib.ERR_INVALID),
         ("ls", -1.0, _lib.ERR_INVALID), ("amplitude", 0.0, _lib.ERR_INVALID), ("param", np.inf, _lib.ERR_INVALID),
         ("y_std", 0.0, _lib.ERR_INVALID), ("k_seeds", 65, _lib.ERR_INVALID), ("best", None, _lib.ERR_INVALID),
         ("X_value", np.nan, _lib.ERR_INVALID), ("candidates", None, _lib.ERR_STATE)]


def call(eng, **wrong):
    a = {**dict(N=40, d=3, kernel=F.MATERN25, n_ls=3, amplitude=1.0, white=0.0, alpha=ALPHA, k=16, acq=T.UCB, param=2.0, y_mean=Y_MEAN,
                y_std=Y_STD, k_seeds=0, ls=0.5, X_value=0.5), **wrong}
    X, y, ls = np.full((40, 3), a["X_value"]) + np.arange(120).reshape(40, 3) / 500.0, np.zeros(40), np.full(3, a["ls"])
    bi, bv = np.empty(1, dtype=np.int64), np.empty(1)
    return eng._lib.gpnn_acq_argbest(eng._h, None if "X" in wrong else dptr(X), dptr(y), a["N"], a["d"], a["kernel"], dptr(ls), a["n_ls"],
                                     a["amplitude"], a["white"], a["alpha"], a["k"], a["acq"], a["param"], 0.0, a["y_mean"], a["y_std"],
                                     a["k_seeds"], 0, None if "best" in wrong else iptr(bi), dptr(bv), *[None] * 6)


@pytest.mark.parametrize("first", range(len(ORDER)), ids=[o[0] for o in ORDER])
def test_refusals_in_the_headers_order(engine, first):
    engine.set_candidates(np.full((5, 4), 0.5))      # candidates of another dimension: the last entry of the order
    if ORDER[first][0] == "candidates":
        with type(engine)(0) as fresh:      # a new context has none
            assert call(fresh) == call(engine) == _lib.ERR_STATE
        for bad in (dict(white=-1.0), dict(alpha=np.nan), dict(y_mean=np.inf), dict(N=(1 << 20) + 1), dict(k_seeds=-1)):
            assert call(engine, **bad) == _lib.ERR_INVALID, bad
    else:
        assert call(engine, **{n: v for n, v, _rc in ORDER[first:-1]}) == ORDER[first][2]
    engine.set_candidates(np.full((5, 3), 0.5))
    assert call(engine) == _lib.GPBO_OK      # the context is still usable
    with pytest.raises(NotImplementedError, match="device group"):
        GroupEngine.nn_acq_argbest(object.__new__(GroupEngine), None, None, 0, None, 0.0, 16, 0, 0.0)


def test_suggest_local_with_20000_observations(engine):
    """f(x) = -|x - 0.3|^2 on [0, 1]^4, 20 000 uniform observations, Matern-2.5 at a fixed length scale 0.5, alpha 1e-4, UCB over 500
    candidates.  The pick is held to nngp_truth's own over the same candidates; on the CPU, with the reference behind a fake engine,
    that pick's true value is 1.79e-2 below the best observation (no candidate is closer), its lead 7.5e-4: the margin is 2.5e-2."""
    from sklearn.gaussian_process.kernels import Matern

    X = np.random.RandomState(8).uniform(size=(20_000, 4))
    y = -((X - 0.3) ** 2).sum(1)
    drv = B.Driver(engine, X, y, np.array([[0.0, 1.0]] * 4), A.UpperConfidenceBound(kappa=2.576), seed=11,
                   kernel=Matern(nu=2.5, length_scale=0.5, length_scale_bounds="fixed"))
    drv._gp.alpha = 1e-4
    params, info = suggest_local(drv, n_neighbors=32, n_random=500, theta_subset=256, return_info=True)
    x = np.array(list(params.values()))
    assert drv._acquisition_function.i == 0 and list(params) == drv._space.keys and info["subset"].shape == (256,)
    Xc = engine.get_candidate_rows(np.arange(500), 4)
    want = T.nngp(F.MATERN25, X, (y - y.mean()) / y.std(), np.array([0.5]), 1e-4, Xc, 32, T.UCB, 2.576, y.max(), y.mean(), y.std())
    order = np.argsort(want["ys"], kind="stable")
    pick, lead = int(order[0]), float(want["ys"][order[1]] - want["ys"][order[0]])
    assert want["gap"] > 0 and lead > 1e-9 and info["index"] == pick and np.array_equal(x, Xc[pick])
    assert np.array_equal(info["neighbors"], want["nbr"][pick]) and -((x - 0.3) ** 2).sum() >= y.max() - 0.025
    assert max(abs(info["mu"] - want["mu"][pick]), abs(info["sd"] - want["sd"][pick]), abs(-info["value"] - want["ys"][pick])) <= 1e-9
