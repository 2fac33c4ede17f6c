"""GPU (-m gpu): gppf_pfes_argbest against pfes_truth (include/gppf.h in fp64 NumPy) on the device's own fetched mu / sd; the
conventions; device-built fronts against the host staircase of gpbo_sample_paths' values; the refusals in order; suggest_pfes.
The values' bar is the project's 1e-9 + 1e-9 |truth| nats, valid while the truth's own fp64 noise — against pfes_truth.pfes_ext,
mpmath at 30 digits, at the candidate of smallest Z (where -log Z and Q / 2Z cancel most) and at the one of largest value — stays
under a tenth of it; otherwise ten times that noise.  The noise is at most 8.4e-13 over CASES on the oracle's posterior and 1.3e-12
on the device's, so the bar is 1e-9 + 1e-9 |truth|.  The fronts are placed so that the truth's smallest Z_s over all (candidate, draw) pairs
stays >= 1e-250 (asserted; smallest on the oracle's posterior 2.0e-85).  Worst device error observed: 2.1e-12 nats."""
import numpy as np
import pytest

import matern_family_truth as F
import pfes_truth as T
from bayesianoptimization_amd import ParetoOptimizer, _lib, suggest_pfes
from bayesianoptimization_amd._lib import GpboError, dptr, iptr
from bayesianoptimization_amd.thompson import spectral_draw

pytestmark = pytest.mark.gpu

N, D, NOISE, L = 40, 3, 0.1, 128
Y_MEAN, Y_STD = (3.5, -1.0), (0.4, 2.0)
KW = dict(y_mean=Y_MEAN, y_std=Y_STD)
X, _y0 = F.data(N, D, seed=123)
_y1 = np.cos(2.0 * X.sum(1)) - X[:, 0] + 0.1 * np.random.RandomState(7).randn(N)
YN = [(y - y.mean()) / y.std() for y in (_y0, _y1)]
LS = 0.15 * np.sqrt(D) * np.geomspace(0.75, 1.33, D)
XC = np.random.RandomState(543).uniform(size=(16384 + 65, D))
SHIFTS = (2.5, 0.0, -3.0)      # a front's centre in y_std from y_mean: the candidates deep inside it, across it, far above it


def posterior(eng, Xc, noise=NOISE):
    """(mu0, sd0, mu1, sd1) of both slots over Xc, left resident"""
    for j in (0, 1):
        eng.fit(X, YN[j], F.MATERN25, LS, noise, slot=j)
    eng.set_candidates(Xc)
    return sum((tuple(eng.posterior(j, Y_MEAN[j], Y_STD[j])) for j in (0, 1)), ())


def fronts_of(S, mode):
    """(fronts (S, 128, 2), sizes (S,)): front s a staircase of `mode`'s size across 3 y_std, centred at SHIFTS[(s + S) % 3]"""
    sizes = np.resize({"one": [1], "full": [L], "mixed": [1, L, 37, 2, 100, 64, 5]}[mode], S).astype(np.int32)
    fronts = np.zeros((S, L, 2))
    for s, n in enumerate(sizes):
        u = 1.5 * (2.0 * (np.arange(n) + 0.5) / n - 1.0)
        for j, sign in ((0, -1.0), (1, 1.0)):
            fronts[s, :n, j] = Y_MEAN[j] + Y_STD[j] * (SHIFTS[(s + S) % 3] + sign * u)
    return fronts, sizes


def bar_of(post, fronts, sizes, want, zmin):
    probe = {int(np.argmin(zmin)), int(np.argmax(want))}
    noise = max(abs(want[i] - T.pfes_ext(*(p[i] for p in post), fronts, sizes)) for i in probe)
    print(f"the fp64 truth's own noise {noise:.2e} nats; smallest Z {zmin.min():.2e}")
    return np.maximum(1e-9 + 1e-9 * np.abs(want), 10.0 * noise if noise > 1e-10 else 0.0)


CASES = [(257, 64, "mixed"), (257, 17, "full"), (257, 16, "one"), (65, 3, "mixed"), (63, 1, "full"), (1, 1, "one"), (65, 17, "mixed")]


@pytest.mark.parametrize("M,S,mode", CASES)      # M, S, front sizes
def test_values_against_the_truth(engine, debug_engine, monkeypatch, M, S, mode):
    post = posterior(engine, XC[:M])
    fronts, sizes = fronts_of(S, mode)
    bi, bv, si, sv, ys = engine.pfes_argbest(fronts, sizes, k_seeds=min(8, M), return_values=True, **KW)
    want, zmin = T.pfes(*post, fronts, sizes)
    assert zmin.min() >= 1e-250 and want.max() > 0.1 and np.isfinite(ys).all()
    err = np.abs(-ys - want)
    print(f"worst |error| {err.max():.2e} nats at truth {want[err.argmax()]:.3e}; truth in [{want.min():.2e}, {want.max():.2e}]")
    assert (err <= bar_of(post, fronts, sizes, want, zmin)).all()
    order = np.argsort(ys, kind="stable")[:min(8, M)]
    assert bi == order[0] and bv == ys[order[0]] and np.array_equal(si, order) and np.array_equal(sv, ys[order])
    as_list = engine.pfes_argbest([fronts[s, :n] for s, n in enumerate(sizes)], index_offset=1 << 40, return_values=True, **KW)
    assert as_list[0] == bi + (1 << 40) and np.array_equal(as_list[4], ys)
    # A candidate alone has the bits it has among the 257.  The posterior pass takes its GEMV path for one candidate and its MFMA
    # path for 257, with other bits; the debug build's GPBO_SMALL_MAX pins the GEMV path for both, as test_gpu_seams.py does.
    monkeypatch.setenv("GPBO_SMALL_MAX", "1024")
    post = posterior(debug_engine, XC[:M]) if M == 257 else None
    ys = debug_engine.pfes_argbest(fronts, sizes, return_values=True, **KW)[4] if M == 257 else None
    for i in (0, 100, 256) if M == 257 else ():
        alone = posterior(debug_engine, XC[i:i + 1])
        assert all(a[0] == p[i] for a, p in zip(alone, post)), "the posterior pass itself depends on M"
        assert debug_engine.pfes_argbest(fronts, sizes, return_values=True, **KW)[4][0] == ys[i]


@pytest.mark.parametrize("what", ["sd0", "nan", "far"])
def test_conventions(engine, what):
    fronts, sizes = fronts_of(17, "mixed")
    if what == "sd0":      # candidates ON the training points of a noise-free fit: sd == 0 (a flagged clip), the step function
        post = posterior(engine, np.vstack([X, XC[:33]]), noise=0.0)
        engine.take_negative_variance_flag()
        assert (post[1] == 0).any() and (post[3] == 0).any() and not (post[1] == 0).all()
        ys = engine.pfes_argbest(fronts, sizes, return_values=True, **KW)[4]
        want = T.pfes(*post, fronts, sizes)[0]
        assert np.isfinite(ys).all() and (np.abs(-ys - want) <= 1e-9 + 1e-9 * np.abs(want)).all()
    elif what == "nan":
        Xn = XC[:130].copy()
        Xn[[77, 11], [1, 0]] = np.nan
        posterior(engine, Xn)
        bi, bv, _si, _sv, ys = engine.pfes_argbest(fronts, sizes, return_values=True, **KW)
        assert bi == 11 and np.isnan(bv) and np.isnan(ys[[11, 77]]).all() and np.isfinite(np.delete(ys, [11, 77])).all()
    else:                  # front 0 sixty sd below every candidate in both objectives: Z = 0, the draw contributes exactly 0
        post = posterior(engine, XC[:65])
        low = [min(Y_MEAN[j] + Y_STD[j] * -9.0, float((post[2 * j] - 60.0 * post[2 * j + 1]).min())) for j in (0, 1)]
        fronts[0, 0], sizes[0] = low, 1
        ys = engine.pfes_argbest(fronts, sizes, return_values=True, **KW)[4]
        rest = engine.pfes_argbest(fronts[1:], sizes[1:], return_values=True, **KW)[4]
        assert np.isfinite(ys).all() and np.allclose(ys * 17.0, rest * 16.0, rtol=1e-14, atol=0.0)


def draws_of(S_g, G, F_n, seed):
    rs = np.random.RandomState(seed)
    one = lambda: spectral_draw(F.MATERN25, F_n, D, rs) + (rs.standard_normal((S_g, F_n)), rs.standard_normal((S_g, N)) * np.sqrt(NOISE))  # noqa: E731
    return [[one() for _ in range(G)] for _ in (0, 1)]


@pytest.mark.parametrize("M", [300, 16384 + 65])
def test_fronts_built_on_the_device(engine, M):
    posterior(engine, XC[:M])
    draws, B = draws_of(3, 2, 64, seed=M), min(M, 16384)
    ys, size, fronts = engine.pfes_argbest(draws=draws, return_values=True, return_fronts=True, **KW)[4:]
    vals = [np.vstack([engine.sample_paths(*g, slot=j, y_mean=Y_MEAN[j], y_std=Y_STD[j], return_values=True)[2] for g in draws[j]])
            for j in (0, 1)]
    for t in range(6):
        want = T.staircase(vals[0][t, :B], vals[1][t, :B])
        assert size[t] == len(want) and np.array_equal(fronts[t, :size[t]], want)
    assert size.max() > 1
    assert np.array_equal(engine.pfes_argbest(fronts, size, return_values=True, **KW)[4], ys)


GOOD = fronts_of(5, "mixed")
bad = lambda at, v: (np.where(np.arange(GOOD[0].size).reshape(GOOD[0].shape) == at, v, GOOD[0]), GOOD[1])      # noqa: E731
REFUSALS = [((np.zeros((0, L, 2)), np.zeros(0)), {}, "n_samples"), ((np.zeros((65, L, 2)), np.ones(65)), dict(k_seeds=65), "n_samples"),
            (GOOD, dict(k_seeds=65, y_std=(np.nan, 1.0)), "k_seeds"), (bad(2, np.nan), dict(y_std=(0.4, 0.0)), "y_std must be finite"),
            (bad(2, np.nan), dict(y_mean=(np.inf, 0.0)), "y_std must be finite"), ((GOOD[0], [1, 0, 3, 2, 5]), {}, "front size"),
            ((GOOD[0], [1, L + 1, 3, 2, 5]), {}, "front size"), (bad(L * 2 + 2, np.inf), dict(y_std=(0.5, 2.0)), "must be finite"),
            (bad(L * 2 + 2, GOOD[0][1, 0, 0]), dict(y_std=(0.5, 2.0)), "strictly"), (bad(L * 2 + 3, GOOD[0][1, 0, 1]), {}, "strictly"),
            (GOOD, dict(y_std=(0.4, 2.5)), "not the one")]


@pytest.mark.parametrize("fronts,kw,match", REFUSALS)
def test_refusals_in_the_stated_order(engine, fronts, kw, match):
    post = posterior(engine, XC[:65])
    with pytest.raises(ValueError, match=match):
        engine.pfes_argbest(*fronts, **{**KW, **kw})
    assert np.array_equal(engine.posterior(0, Y_MEAN[0], Y_STD[0])[0], post[0])      # the context stays usable


def test_refusals_of_state_pointers_and_draw_counts(engine):
    eng = engine
    posterior(eng, XC[:65])
    fr, sz, ym, ys_, bi, bv = GOOD[0], GOOD[1].ctypes.data_as(_lib._c_int_p), np.array(Y_MEAN), np.array(Y_STD), np.empty(1, dtype=np.int64), np.empty(1)
    call = lambda *a: eng._lib.gppf_pfes_argbest(eng._h, *a)      # noqa: E731
    tail = (0, 0, iptr(bi), dptr(bv), None, None, None, None, None)
    assert call(dptr(ym), dptr(ys_), 0, 0, 0, None, None, None, None, 5, None, dptr(fr), *tail) == _lib.ERR_INVALID
    assert call(None, dptr(ys_), 0, 0, 0, None, None, None, None, 5, sz, dptr(fr), *tail) == _lib.ERR_INVALID
    assert call(dptr(ym), dptr(ys_), 0, 0, 0, None, None, None, None, 5, sz, dptr(fr), 0, 0, None, *tail[3:]) == _lib.ERR_INVALID
    for G, S_g, F_n in ((0, 3, 64), (17, 3, 64), (2, 17, 64), (2, 3, 4097), (5, 13, 64)):      # device-front mode's counts; 65 draws
        assert call(dptr(ym), dptr(ys_), G, S_g, F_n, dptr(fr), dptr(fr), dptr(fr), dptr(fr), 0, None, None, *tail) == _lib.ERR_INVALID
    assert call(dptr(ym), dptr(ys_), 2, 3, 64, dptr(fr), None, dptr(fr), dptr(fr), 0, None, None, *tail) == _lib.ERR_INVALID
    assert call(dptr(ym), dptr(ys_), 0, 0, 0, None, None, None, None, 5, sz, dptr(fr), *tail) == _lib.GPBO_OK
    eng.set_candidates(XC[:40])
    eng.posterior(0, Y_MEAN[0], Y_STD[0], fetch=False)
    with pytest.raises(GpboError, match="run gpbo_posterior for both objectives' slots first"):      # slot 1 has none yet
        eng.pfes_argbest(*GOOD, **KW)
    eng.posterior(1, Y_MEAN[1], Y_STD[1], fetch=False)
    with eng.overlapped_fits():
        eng.fit(X, YN[1], F.MATERN25, LS, NOISE, slot=1)
        assert call(dptr(ym), dptr(ys_), 0, 0, 0, None, None, None, None, 5, sz, dptr(fr), *tail) == _lib.ERR_STATE


def test_suggest_pfes_end_to_end(engine):
    bounds = {"a": (0.0, 1.0), "b": (-1.0, 2.0), "c": (0.5, 1.5)}
    lo, hi = np.array(list(bounds.values())).T
    Xo = lo + np.random.RandomState(0).uniform(size=(30, 3)) * (hi - lo)
    Yo = np.column_stack([np.sin(3.0 * Xo[:, 0]) * np.cos(2.0 * Xo[:, 1]) + Xo[:, 2] ** 2, -((Xo[:, 0] - 0.7) ** 2) - 0.3 * Xo[:, 1]]) \
        + 0.05 * np.random.RandomState(1).standard_normal((30, 2))

    def run(m=2, **kw):
        opt = ParetoOptimizer(bounds, m, [-1.5] * m, n_restarts_optimizer=2, random_state=11, engine=engine, alpha=1e-2, **kw)
        for x, y in zip(Xo, Yo):
            opt.register(x, np.resize(y, m), **({"constraint_values": [0.0]} if kw else {}))
        return opt, suggest_pfes(opt, n_random=257, n_samples=20, n_features=128, return_info=True)

    opt, (params, info) = run()
    x = np.array([params[k] for k in bounds])
    assert list(params) == list(bounds) and (x >= lo).all() and (x <= hi).all() and info["value"] > 0.0
    assert info["n_samples"] == 20 and info["front_size"].shape == (20,) and (info["front_size"] >= 1).all()
    assert np.array_equal(x, engine.get_candidate_rows(np.array([info["index"]]), 3)[0])
    again, (params2, info2) = run()
    assert params2 == params and info2["index"] == info["index"]
    assert all(np.array_equal(a, b) for a, b in zip(opt._random_state.get_state()[1:3], again._random_state.get_state()[1:3]))
    for kw in (dict(m=3), dict(constraints=[(-1.0, 1.0)])):
        with pytest.raises(NotImplementedError, match="suggest_pfes"):
            run(**kw)
