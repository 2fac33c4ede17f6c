"""GPU (-m gpu): gpmf_mes_argbest against include/gpmf.h restated in NumPy (q, q', x, m' from an fp64 Cholesky written out, r2 from
jes_truth), a candidate's bits alone and among 257, the degenerate pair, conventions, reader contract, refusals, suggest_multifidelity.
Bars: max(1e-9, 4 D) absolute for ys (nats per cost), rho, m' and sqrt(vg) (normalised units), D the fp64 truth's own distance from its
np.longdouble twin, printed.  The fixtures are asserted, from the truth alone, to have >= 10 % of the candidates at a >= 1e-3, at
|rho| < 0.9 and at |rho| > 0.5, and cond(K) <= 1e6: otherwise the cross term is not really tested."""
import functools

import numpy as np
import pytest

import batch_truth as B
import jes_truth as T
import matern_family_truth as F
from bayesianoptimization_amd import _lib
from bayesianoptimization_amd import _suggest
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd import suggest_multifidelity
from bayesianoptimization_amd._lib import GpboError, dptr, iptr
from bayesianoptimization_amd.engine import GpEngine, GroupEngine
from bayesianoptimization_amd.thompson import spectral_draw
from mes_truth import argbest

pytestmark = pytest.mark.gpu

Y_MEAN, Y_STD, TARGET, COST0 = 3.5, 0.4, 1.0, 0.5
KW = dict(y_mean=Y_MEAN, y_std=Y_STD)
#        N, d, M, kind, fid_col, S, cost1 [, c, w, alpha]: one ragged stage | three 64-row pads | across a 256-row chunk | three chunks
CASES = {"n40": (40, 2, 257, F.MATERN25, 0, 16, 0.0), "n130": (130, 5, 130, F.MATERN15, 2, 17, 0.5),
         "n300": (300, 5, 257, F.RBF, 1, 1, 0.0), "n530": (530, 5, 130, F.MATERN05, 4, 64, 2.0),
         "scaled": (40, 3, 257, F.MATERN25, 1, 16, 0.5, 2.5, 0.03, 1e-3)}


class Case:
    def __init__(self, N, d, M, kind, fid, S, cost1, c=1.0, w=0.0, alpha=1e-3):
        self.N, self.d, self.M, self.kind, self.fid, self.S, self.cost1, self.c, self.w, self.alpha = N, d, M, kind, fid, S, cost1, c, w, alpha
        self.X, y = F.data(N, d, seed=3 * N + d)
        self.yn = (y - y.mean()) / y.std()
        self.ls = (0.3 if d > 2 else 0.1) * np.sqrt(d) * np.geomspace(0.75, 1.33, d)      # ARD; short in 2-D, where 40 points would pin f
        self.ls[fid] *= 2.5                                           # fidelities correlate: |rho| spreads over (0, 1)
        self.Xc = np.random.RandomState(500 + N + d).uniform(size=(M, d))
        self.y_star = Y_STD * (self.yn.max() - 1.0 + np.linspace(0.0, 1.2, S)) + Y_MEAN

    def fit(self, eng, Xc=None):
        eng.fit(self.X, self.yn, self.kind, self.ls, self.alpha, **({} if self.c == 1.0 else dict(amplitude=self.c, white=self.w)))
        eng.set_candidates(self.Xc if Xc is None else Xc)

    def call(self, eng, **kw):
        return eng.mf_mes_argbest(self.y_star, self.fid, TARGET, COST0, self.cost1, return_values=True, return_parts=True, **{**KW, **kw})

    def truth(self, Xc=None, dtype=np.float64, r2_of=T.r2):
        """(a / cost, rho, m', sqrt(vg)) of include/gpmf.h, normalised units; the factorisation and the solves in `dtype`"""
        Xc = self.Xc if Xc is None else Xc
        eta, S = (self.w + self.alpha) / self.c, len(self.y_star)
        Zt = np.where(np.arange(self.d) == self.fid, TARGET, Xc)
        K = F.kernel_matrix(self.kind, self.X, None, self.ls).astype(dtype)
        K[np.diag_indices_from(K)] += dtype(eta)
        Bm = np.column_stack([F.kernel_matrix(self.kind, self.X, Xc, self.ls), F.kernel_matrix(self.kind, self.X, Zt, self.ls), self.yn]).astype(dtype)
        L = np.zeros_like(K)
        for j in range(len(K)):                                      # Cholesky, then L^-1 B by forward substitution
            L[j, j] = np.sqrt(K[j, j] - L[j, :j] @ L[j, :j])
            L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
        for i in range(len(K)):
            Bm[i] = (Bm[i] - L[i, :i] @ Bm[:i]) / L[i, i]
        M = len(Xc)
        U, Ut, wy = Bm[:, :M], Bm[:, M:2 * M], Bm[:, -1]
        q, qt, x, mp = (np.asarray(t, dtype=np.float64) for t in ((U * U).sum(0), (Ut * Ut).sum(0), (U * Ut).sum(0), Ut.T @ wy))
        s = Xc[:, self.fid]
        with np.errstate(all="ignore"):
            vl, vg = self.c * np.maximum(1 - q, 0), self.c * np.maximum(1 - qt, 0)
            cv = self.c * (F.kernel_value(self.kind, np.abs(s - TARGET) / self.ls[self.fid]) - x)
            vo = vl + self.c * eta
            ok = (vo > 0) & (vg > 0)
            rho2 = np.where(ok, np.minimum(cv * cv / np.where(ok, vo * vg, 1.0), 1.0), 0.0)
            gam = ((self.y_star - Y_MEAN) / Y_STD - mp[:, None]) / np.sqrt(vg)[:, None]
            acc = np.zeros(M)
            for k in range(S):
                ratio = np.array([1.0 if (r == 0 or np.isnan(g)) else r2_of(g) for g, r in zip(gam[:, k], rho2)])
                acc = acc + np.log1p(-(rho2 * (1 - ratio)))
            a = np.where(ok, -(acc / (2 * S)), 0.0)
            cost = COST0 + self.cost1 * s
            ys = np.where(np.isnan(q + qt + x + mp) | ~((cost > 0) & np.isfinite(cost)), np.nan, a / cost)
        return ys, np.copysign(np.sqrt(rho2), cv), mp, np.sqrt(vg), a

    def cond(self):
        return np.linalg.cond(F.kernel_matrix(self.kind, self.X, None, self.ls) + (self.w + self.alpha) / self.c * np.eye(self.N))


case_of = functools.lru_cache(maxsize=None)(lambda name: Case(*CASES[name]))


def check(what, got, want, D):
    """got = (ys, rho, mu_t, sd_t) of the device, want / D the truth's and its own noise, each in the header's units"""
    got = (-got[0], got[1], (got[2] - Y_MEAN) / Y_STD, got[3] / Y_STD)
    for n, g, t, dd in zip(("ys", "rho", "m'", "sqrt(vg)"), got, want, D):
        assert np.array_equal(np.isnan(g), np.isnan(t)), n
        worst, bar = float(np.nanmax(np.abs(g - t))), max(1e-9, 4.0 * dd)
        print(f"{what} {n}: worst |error| = {worst:.2e}, the truth's own noise D = {dd:.2e}, bar {bar:.1e}")
        assert worst <= bar, f"{what} {n}: {worst:.2e} over the bar {bar:.1e}"


def noise_of(c, Xc=None, t64=None):
    t64, tld = t64 or c.truth(Xc), c.truth(Xc, np.longdouble)
    return [float(np.nanmax(np.abs(a - b))) for a, b in zip(t64[:4], tld[:4])]


@pytest.mark.parametrize("name", list(CASES))
def test_values_and_selection(engine, name):
    c = case_of(name)
    want = c.truth()
    a, rho = want[4], np.abs(want[1])
    print(f"{name}: cond(K) = {c.cond():.1e}; shares a >= 1e-3: {np.mean(a >= 1e-3):.2f}, |rho| < 0.9: {np.mean(rho < 0.9):.2f}, |rho| > 0.5: {np.mean(rho > 0.5):.2f}")
    assert c.cond() <= 1e6 and min(np.mean(a >= 1e-3), np.mean(rho < 0.9), np.mean(rho > 0.5)) >= 0.10, "this fixture does not test the cross term"
    c.fit(engine)
    bi, bv, si, sv, ys, *parts = c.call(engine, k_seeds=8)
    check(name, (ys, *parts), want, noise_of(c, t64=want))
    wi, wv, wsi, wsv = argbest(ys, 8)
    assert bi == wi and bv == wv and np.array_equal(si, wsi) and np.array_equal(sv, wsv)
    oi, ov, osi, osv = c.call(engine, k_seeds=8, index_offset=10_000_000_000)[:4]
    assert oi == bi + 10_000_000_000 and ov == bv and np.array_equal(osi, si + 10_000_000_000) and np.array_equal(osv, sv)


@pytest.mark.parametrize("name", ["n40", "n300"])
def test_a_candidate_alone_has_the_bits_it_has_among_257(engine, name):
    c = case_of(name)
    c.fit(engine)
    many = c.call(engine)[4:]
    for row in (0, 100, 256):
        c.fit(engine, c.Xc[row:row + 1])
        for alone, among in zip(c.call(engine)[4:], many):
            assert alone[0] == among[row] or (np.isnan(alone[0]) and np.isnan(among[row]))


def test_degenerate_pair(engine):
    """z' = z: rho^2 = vg / (vg + lambda); with lambda tiny and c = 1, rho^2 -> 1 and a = -1/2 mean log r2(gamma) (not MES's h)"""
    c = case_of("n40")
    Xc = c.Xc.copy()
    Xc[:, c.fid] = TARGET
    c.fit(engine, Xc)
    ys, rho, mu_t, sd_t = c.call(engine)[4:]
    want = c.truth(Xc)
    check("degenerate", (ys, rho, mu_t, sd_t), want, noise_of(c, Xc, want))
    vg = (sd_t / Y_STD) ** 2
    assert np.abs(rho ** 2 - vg / (vg + c.alpha)).max() <= 1e-9
    t = Case(*CASES["n40"], alpha=1e-12)
    t.fit(engine, Xc)
    ys, rho, mu_t, sd_t = t.call(engine)[4:]
    gam = (t.y_star - mu_t[:, None]) / sd_t[:, None]
    a = -0.5 * np.mean(np.log([[T.r2(g) for g in row] for row in gam]), axis=1)
    live = sd_t / Y_STD > 1e-3                                  # rho^2 = vg / (vg + 1e-12) is 1 to 1e-6 there
    assert live.mean() > 0.5 and np.abs(-ys * COST0 - a)[live].max() <= 1e-5


def test_conventions(engine):
    """a NaN coordinate wins; a cost <= 0 is NaN; vg == 0 (a training point at the target fidelity, no noise) gives a = 0"""
    c = case_of("scaled")                                       # cost1 = 0.5
    Xn = c.Xc.copy()
    Xn[[140, 11], [2, c.fid]] = np.nan
    Xn[[30, 31], c.fid] = -1.5, -1.0                            # cost = 0.5 - 0.75 | 0
    c.fit(engine, Xn)
    bi, bv, si, sv, ys, rho, mu_t, sd_t = c.call(engine, k_seeds=8)
    assert bi == 11 and np.isnan(bv) and np.isnan(ys[[11, 30, 31, 140]]).all() and np.isfinite(np.delete(ys, [11, 30, 31, 140])).all()
    assert np.isfinite(rho[[30, 31]]).all() and np.isnan(rho[[11, 140]]).all()
    t = Case(*CASES["n40"], alpha=0.0)
    t.X[:20, t.fid] = TARGET
    Xc = np.vstack([t.X[:20], t.Xc[:13]])
    t.fit(engine, Xc)
    ys, rho, mu_t, sd_t = t.call(engine)[4:]
    print(f"vg == 0 at {int((sd_t == 0).sum())} of the 20 training points")
    assert (sd_t[:20] == 0).any() and (ys[sd_t == 0] == 0).all() and (rho[sd_t == 0] == 0).all() and not np.isnan(ys).any()


def test_reader_only(engine):
    eng, c = engine, case_of("n130")
    c.fit(eng)
    eng.posterior(0, Y_MEAN, Y_STD, fetch=False)
    eng.take_negative_variance_flag()
    before = eng.mes_argbest(c.y_star[:4], k_seeds=8, return_values=True)
    c.call(eng, k_seeds=8)
    after = eng.mes_argbest(c.y_star[:4], k_seeds=8, return_values=True)      # the resident mu / sd still serve
    assert before[0] == after[0] and before[1] == after[1] and all(np.array_equal(a, b) for a, b in zip(before[2:], after[2:]))
    assert np.array_equal(eng.get_candidate_rows(np.arange(c.M), c.d), c.Xc) and eng.take_negative_variance_flag() is False


GOOD = np.full(5, 4.0)      # REFUSALS: y_star, fid_col, fid_target, cost0, cost1, kw, match — the NEXT check's argument bad too
REFUSALS = [(np.zeros(0), 64, 1.0, 1.0, 0.0, {}, "n_samples"), (np.zeros(65), 0, 1.0, 1.0, 0.0, {}, "n_samples"),
            (np.where(np.arange(5) == 2, np.nan, GOOD), -1, 1.0, 1.0, 0.0, {}, "y_star must be finite"),
            (GOOD, -1, np.nan, 1.0, 0.0, {}, "fid_col"), (GOOD, 64, 1.0, 1.0, 0.0, {}, "fid_col"),
            (GOOD, 0, np.inf, 0.0, 0.0, {}, "fid_target"), (GOOD, 0, 1.0, 0.0, -1.0, {}, "cost0"), (GOOD, 0, 1.0, np.inf, 0.0, {}, "cost0"),
            (GOOD, 0, 1.0, 1.0, -1.0, dict(k_seeds=65), "cost1"), (GOOD, 0, 1.0, 1.0, np.nan, {}, "cost1"),
            (GOOD, 0, 1.0, 1.0, 0.0, dict(k_seeds=65, y_std=np.nan), "k_seeds"), (GOOD, 0, 1.0, 1.0, 0.0, dict(y_std=0.0), "y_std"),
            (GOOD, 0, 1.0, 1.0, 0.0, dict(y_mean=np.inf), "y_std"), (GOOD, 3, 1.0, 1.0, 0.0, {}, "not a column")]


@pytest.mark.parametrize("y_star,fid,target,cost0,cost1,kw,match", REFUSALS)
def test_refusals_in_the_stated_order(engine, y_star, fid, target, cost0, cost1, kw, match):
    case_of("n40").fit(engine)
    with pytest.raises(ValueError, match=match):
        engine.mf_mes_argbest(y_star, fid, target, cost0, cost1, **{**KW, **kw})


def test_refusals_of_state_and_pointers(engine):
    eng, c = engine, case_of("n40")
    c.fit(eng)
    bi, bv, sv, call, y, tail = np.empty(1, dtype=np.int64), np.empty(1), np.empty(4), eng._lib.gpmf_mes_argbest, dptr(GOOD), (None,) * 4
    assert call(eng._h, 0, 1.0, 1.0, 0.0, None, 5, Y_MEAN, Y_STD, 0, 0, iptr(bi), dptr(bv), None, None, *tail) == _lib.ERR_INVALID
    assert call(eng._h, 0, 1.0, 1.0, 0.0, y, 5, Y_MEAN, Y_STD, 0, 0, None, dptr(bv), None, None, *tail) == _lib.ERR_INVALID
    assert call(eng._h, 0, 1.0, 1.0, 0.0, y, 5, Y_MEAN, Y_STD, 4, 0, iptr(bi), dptr(bv), None, dptr(sv), *tail) == _lib.ERR_INVALID
    assert call(eng._h, 0, 1.0, 1.0, 0.0, y, 5, Y_MEAN, Y_STD, 0, 0, iptr(bi), dptr(bv), None, None, *tail) == _lib.GPBO_OK
    eng.set_candidates(np.zeros((10, 4)))
    with pytest.raises(GpboError, match="dimension differs"):
        eng.mf_mes_argbest(GOOD, 0, 1.0, **KW)
    eng.set_candidates(c.Xc)
    with eng.overlapped_fits():
        eng.fit(c.X, c.yn, c.kind, c.ls, c.alpha)
        rc = call(eng._h, 0, 1.0, 1.0, 0.0, y, 5, Y_MEAN, Y_STD, 0, 0, iptr(bi), dptr(bv), None, None, *tail)
        assert rc == _lib.ERR_STATE
        with pytest.raises(GpboError, match="pending gpbo_fit_begin"):
            eng._check(rc)
    with GpEngine(0) as fresh:
        with pytest.raises(GpboError, match="not been fitted"):
            fresh.mf_mes_argbest(GOOD, 0, 1.0, **KW)
        fresh.fit(c.X, c.yn, c.kind, c.ls, c.alpha)
        with pytest.raises(GpboError, match="no candidates"):
            fresh.mf_mes_argbest(GOOD, 0, 1.0, **KW)
    with pytest.raises(NotImplementedError, match="device group"):
        GroupEngine.mf_mes_argbest(object.__new__(GroupEngine), GOOD, 0, 1.0)


def test_suggest_multifidelity_end_to_end(engine):
    """two parameters + a fidelity in [0.01, 1], exact at 1 and slightly biased below.  FEW observations (12) and a long fidelity length
    scale (fixed kernel): (x, s) stays correlated with (x, 1); with dense data rho^2 at s = 0.01 is < 0.03 and no cost moves the pick"""
    from sklearn.gaussian_process.kernels import Matern

    N, M, F_, NS = 12, 20_000, 64, 5
    bounds = np.array([[0.0, 1.0], [0.01, 1.0], [-1.0, 2.0]])      # keys sort as a, fid, z: the fidelity is the MIDDLE column
    rs = np.random.RandomState(77)
    X = bounds[:, 0] + rs.uniform(size=(N, 3)) * (bounds[:, 1] - bounds[:, 0])
    y = np.sin(2.0 * X[:, 0]) + 0.5 * np.cos(1.5 * X[:, 2]) - 0.1 * (1.0 - X[:, 1]) * X[:, 0] + 0.05 * rs.standard_normal(N)

    def driver():
        drv = B.Driver(engine, X, y, bounds, A.UpperConfidenceBound(kappa=2.576), seed=11, n_random=M, optimizer=None,
                       kernel=Matern(nu=2.5, length_scale=[0.4, 2.0, 0.8]))
        drv._gp.alpha = 1e-2
        return drv

    drv = driver()
    name = drv._space.keys[1]
    kw = dict(n_samples=NS, n_random=M, n_star=500, n_features=F_, return_info=True)
    flat, info = suggest_multifidelity(drv, name, cost=(1.0, 0.0), **kw)
    x = np.array(list(flat.values()))
    assert list(flat) == drv._space.keys and (x >= bounds[:, 0]).all() and (x <= bounds[:, 1]).all()
    assert info["value"] >= 0 and info["y_star"].shape == (NS,) and 0.0 <= abs(info["rho"]) <= 1.0 and info["cost"] == 1.0
    # the RandomState ends where the docstring says: 2 x uniform(n_star), the draws of one group, 3 x uniform(M)
    twin = driver()
    _suggest.fit_model(twin._gp, twin._space, "twin")
    r = twin._random_state
    for t in (0, 2):
        r.uniform(bounds[t, 0], bounds[t, 1], 500)
    spectral_draw(twin._gp._kind, F_, 3, r)
    r.standard_normal((NS, F_))
    r.standard_normal((NS, N))
    for t in range(3):
        r.uniform(bounds[t, 0], bounds[t, 1], M)
    assert B.same_state(drv._random_state, r)
    # flat cost: a rises with rho^2 and rho^2 with s: the top tenth of the range (no nearer: Matern-2.5 is flat at 0, rho^2 at 0.9 is
    # 0.4 % under the target's); off the data vg >= 0.1, lambda = 0.01: rho^2 = vg / (vg + lambda) >= 0.91.  A cost rising 100-fold
    # where rho^2 falls < 10-fold (the prior's kappa(0.99 / 2)^2 = 0.69): best at the low end.  The header in NumPy, 30 seeds: >= 0.93, <= 0.02
    steep, steep_info = suggest_multifidelity(driver(), name, cost=(1e-3, 10.0), **kw)
    print(f"flat cost: fidelity {flat[name]:.3f}, rho {info['rho']:.3f}; steep cost: fidelity {steep[name]:.3f}, rho {steep_info['rho']:.3f}")
    assert flat[name] > 0.9 and abs(info["rho"]) > 0.95
    assert steep[name] < 0.3 and np.array_equal(steep_info["y_star"], info["y_star"])
    assert suggest_multifidelity(driver(), name, fidelities=[0.25, 0.5, 1.0], **kw)[0][name] in (0.25, 0.5, 1.0)
