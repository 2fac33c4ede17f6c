"""GPU (-m gpu): gpbo_posterior_refresh — the resident posterior brought up to date after gpbo_fit_append by one k* generation
against the appended rows of W = L^-1, instead of a full pass.

Every case runs fit, set_candidates, posterior, fit_append, posterior_refresh and asserts
  * route 1 (the incremental update ran);
  * mu / sd against the oracle's from-scratch refit of all rows through test_gpu_sizes.check_posterior at that suite's bars for an
    appended model: 1e-9 (the Matern kinds) / 1e-6 (RBF) max-norm, 1e-5 per candidate;
  * the same bars against the device's own gpbo_posterior on the same slot straight after;
  * gpbo_acq_argbest (UCB, EI, POI, k = 16) after the refresh against the one after the full pass: same best index, same top 16,
    values within 1e-8.  The best index is a well-posed question only where the oracle's own best and second value are further
    apart than rounding: the test asserts (second - best) / max |value| >= 1e-6 on the oracle ALONE — the seeds below were picked
    on the CPU so that it holds in every case; none is skipped for it.
The shapes are the edges of the code, not the workload: the one-launch fit tier with M not a block multiple; a 64-row pad filled
exactly (a further row must report route 0); 16 rows, the most the incremental route takes (17 must report route 0); the strip /
blocked tier edge; NP = 2048 at the widest d.  Length scales and data come from test_gpu_sizes (its factor table per kernel class
and N tier, the nearest d of the table), noise 1e-6.  Further: 16 chained single-row appends with no full pass in between, a
scaled slot, an F32 slot at test_gpu_f32's bars, an append of targets only, and "never stale": every other writer of the slot or
of the candidates makes the next refresh the full pass, bit for bit."""
import functools

import numpy as np
import pytest

import matern_family_truth as F
import scaled_kernel_truth as SK
import test_gpu_sizes as S
from bayesianoptimization_amd import sobol_tables
from bayesianoptimization_amd._lib import GpboError
from bayesianoptimization_amd.engine import F32
from conftest import rel_err
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

NOISE = S.NOISE
KNAME = {F.RBF: "rbf", F.MATERN25: "matern25", F.MATERN15: "matern15", F.MATERN05: "matern05"}
ACQS = ((O.UCB, 2.576), (O.EI, 0.01), (O.POI, 0.3))      # (xi = 0.3: at 0.01 POI saturates at 1.0 on whole sets of RBF candidates — exact ties)
GAP_FLOOR = 1e-6
SPARE = 17          # rows kept beyond a case's own: the appends that must fall back to the full pass

#: (N0, d, M, rows appended, one length scale per dimension)
SHAPES = {
    "one-launch": (5, 1, 257, 1, False),
    "pad-filled": (60, 3, 5000, 4, False),
    "16-rows": (130, 16, 4097, 16, True),
    "strip-edge": (1000, 8, 3000, 8, False),
    "np2048-d64": (2040, 64, 1025, 3, False),
}
ALL_KINDS = (F.RBF, F.MATERN25, F.MATERN15, F.MATERN05)
CASES = [(s, k) for s in ("one-launch", "pad-filled", "16-rows") for k in ALL_KINDS] + \
        [(s, k) for s in ("strip-edge", "np2048-d64") for k in (F.MATERN25, F.RBF)]
#: data seed per case where the default (0) leaves the oracle's best and second acquisition value closer than GAP_FLOOR
SEED = {("one-launch", F.MATERN25): 8, ("one-launch", F.MATERN15): 6, ("pad-filled", F.RBF): 5}


def tol_of(kind):
    return 1e-6 if kind == F.RBF else 1e-9


def length_scale(kind, d, per_dim, N):
    """test_gpu_sizes.length_scale for a (kernel kind, d) outside its table: the factor of the kernel's class (RBF, or Matern
    nu = 2.5 for the three Matern kinds) at the table's nearest d and this N's tier, times sqrt(d)."""
    cls = O.RBF if kind == F.RBF else O.MATERN25
    key = next(k for k in S.LS_FACTOR if k[0] == cls and k[1] == (5 if d <= 10 else 17))
    f = S.LS_FACTOR[key][next(i for i, n in enumerate(S.TIERS) if N <= n)]
    s = f * np.sqrt(d)
    return s * np.geomspace(0.75, 1.33, d) if per_dim else np.array([s])


class Case:
    """Data of one case, the oracle's posterior after the append and the oracle's acquisition gaps (computed once, shared)."""

    def __init__(self, N0, d, M, rows, per_dim, kind, seed=0):
        self.N0, self.d, self.M, self.rows, self.kind = N0, d, M, rows, kind
        self.N = N0 + rows
        self.X, self.y, self.Xc = S.make_data(self.N + SPARE, d, seed * 7919 + 31 * N0 + d + kind, M)
        self.ls = length_scale(kind, d, per_dim, self.N)
        self.what = f"N0={N0}+{rows} {KNAME[kind]} d={d} M={M}"

    def norm(self, n):
        return O.normalize_targets(self.y[:n])

    def truth(self, n, y=None):
        """(mu, sd) of the oracle's from-scratch fit of the first n rows, in the targets' units"""
        yn, ym, ys = O.normalize_targets(self.y[:n] if y is None else y)
        gp = F.fit_fixed_theta(self.kind, self.X[:n], yn, self.ls, NOISE, normalize_y=False)
        mu, sd = F.predict(gp, self.Xc)
        return ys * mu + ym, ys * sd

    def gaps(self, mu, sd, n):
        y_max = float(np.max(self.y[:n]))
        out = []
        for acq, param in ACQS:
            with np.errstate(all="ignore"):
                v = -1 * O.base_acq(acq, mu, sd, param, y_max)
            two = np.partition(v, 1)[:2]
            out.append(float((two[1] - two[0]) / np.max(np.abs(v))))
        return out


@functools.lru_cache(maxsize=None)
def case_of(shape, kind):
    c = Case(*SHAPES[shape], kind, seed=SEED.get((shape, kind), 0))
    c.mu_o, c.sd_o = c.truth(c.N)
    c.gap = c.gaps(c.mu_o, c.sd_o, c.N)
    return c


def arm(eng, c, precision=0, **scaled):
    """fit the first N0 rows, make the candidates resident, run the full posterior: the state an append starts from"""
    yn, ym, ys = c.norm(c.N0)
    eng.fit(c.X[:c.N0], yn, c.kind, c.ls, NOISE, precision=precision, **scaled)
    eng.set_candidates(c.Xc)
    eng.posterior(0, ym, ys, fetch=False)


def append(eng, c, n0, n1, **scaled):
    yn, ym, ys = c.norm(n1)
    eng.fit_append(c.X[n0:n1], yn, **scaled)
    return ym, ys


def argbests(eng, c, n):
    y_max = float(np.max(c.y[:n]))
    return [eng.acq_argbest(acq, param, y_max, k_seeds=16, return_values=True) for acq, param in ACQS]


@pytest.mark.parametrize("shape,kind", CASES, ids=[f"{s}-{KNAME[k]}" for s, k in CASES])
def test_refresh_after_append(engine, shape, kind):
    c = case_of(shape, kind)
    tol = tol_of(kind)
    arm(engine, c)
    ym, ys = append(engine, c, c.N0, c.N)
    with pytest.raises(GpboError):                       # an append still ends the resident posterior
        engine.acq_argbest(O.UCB, 2.576, k_seeds=0)
    mu, sd, route = engine.posterior_refresh(0, ym, ys, return_route=True)
    assert route == 1
    print(f"{c.what}: vs oracle mu {rel_err(mu, c.mu_o):.2e} sd {rel_err(sd, c.sd_o):.2e}; oracle gaps {c.gap}")
    S.check_posterior(mu, sd, c.mu_o, c.sd_o, ys, c.what + " refresh vs oracle", tol)
    after_refresh = argbests(engine, c, c.N)
    mu_f, sd_f = engine.posterior(0, ym, ys)
    print(f"{c.what}: vs full pass mu {rel_err(mu, mu_f):.2e} sd {rel_err(sd, sd_f):.2e}")
    S.check_posterior(mu, sd, mu_f, sd_f, ys, c.what + " refresh vs full pass", tol)
    after_full = argbests(engine, c, c.N)
    assert min(c.gap) >= GAP_FLOOR, f"{c.what}: the oracle's own best / second gap {c.gap}: pick another seed"
    for (acq, _), a, b in zip(ACQS, after_refresh, after_full):
        assert a[0] == b[0], f"{c.what} acq {acq}: best index {a[0]} after the refresh, {b[0]} after the full pass"
        assert np.array_equal(a[2], b[2]), f"{c.what} acq {acq}: top 16"
        assert rel_err(a[4], b[4]) <= 1e-8, f"{c.what} acq {acq}: values {rel_err(a[4], b[4]):.2e}"
    # the rows beyond what the incremental route takes: the full pass, reported as such, and exactly gpbo_posterior
    extra = {"pad-filled": 1, "16-rows": 17}.get(shape)
    if extra:
        assert shape != "pad-filled" or c.N % 64 == 0
        ym2, ys2 = append(engine, c, c.N, c.N + extra)
        mu2, sd2, route2 = engine.posterior_refresh(0, ym2, ys2, return_route=True)
        assert route2 == 0
        mu3, sd3 = engine.posterior(0, ym2, ys2)
        assert np.array_equal(mu2, mu3) and np.array_equal(sd2, sd3)
        mu_o, sd_o = c.truth(c.N + extra)
        S.check_posterior(mu2, sd2, mu_o, sd_o, ys2, c.what + f" +{extra} (full pass)", tol)


@pytest.mark.parametrize("shape,kind", [("16-rows", F.MATERN25), ("strip-edge", F.RBF)], ids=["n130-matern25", "n1000-rbf"])
def test_sixteen_chained_refreshes_without_a_full_pass(engine, shape, kind):
    N0, d, M, _, per_dim = SHAPES[shape]
    c = Case(N0, d, M, 16, per_dim, kind)
    arm(engine, c)
    for n in range(N0, N0 + 16):
        ym, ys = append(engine, c, n, n + 1)
        mu, sd, route = engine.posterior_refresh(0, ym, ys, fetch=(n == N0 + 15), return_route=True)
        assert route == 1
    mu_o, sd_o = c.truth(N0 + 16)
    print(f"{c.what} chained: mu {rel_err(mu, mu_o):.2e} sd {rel_err(sd, sd_o):.2e}")
    S.check_posterior(mu, sd, mu_o, sd_o, ys, c.what + " chained", tol_of(kind))
    mu_f, sd_f = engine.posterior(0, ym, ys)
    S.check_posterior(mu, sd, mu_f, sd_f, ys, c.what + " chained vs full pass", tol_of(kind))


def test_scaled_slot(engine):
    amp, white = 2.5, 1e-3
    c = Case(100, 5, 3000, 2, True, F.MATERN25)
    arm(engine, c, amplitude=amp, white=white)
    ym, ys = append(engine, c, c.N0, c.N, amplitude=amp, white=white)
    mu, sd, route = engine.posterior_refresh(0, ym, ys, return_route=True)
    assert route == 1
    yn = c.norm(c.N)[0]
    gp = SK.ScaledGP(c.kind, c.X[:c.N], yn, c.ls, c=amp, w=white, a=NOISE, y_mean=ym, y_std=ys)
    mu_o, sd_o = SK.predict(gp, c.Xc)
    print(f"{c.what} scaled: mu {rel_err(mu, mu_o):.2e} sd {rel_err(sd, sd_o):.2e}")
    S.check_posterior(mu, sd, mu_o, sd_o, ys, c.what + " scaled", 1e-9)
    mu_f, sd_f = engine.posterior(0, ym, ys)
    S.check_posterior(mu, sd, mu_f, sd_f, ys, c.what + " scaled vs full pass", 1e-9)


def test_f32_slot_keeps_the_f32_bars(engine):
    c = Case(300, 5, 5000, 3, False, F.MATERN25)
    arm(engine, c, precision=F32)
    ym, ys = append(engine, c, c.N0, c.N)
    mu, sd, route = engine.posterior_refresh(0, ym, ys, return_route=True)
    assert route == 1
    mu_o, sd_o = c.truth(c.N)
    print(f"{c.what} f32: mu {rel_err(mu, mu_o):.2e} var {np.max(np.abs(sd**2 - sd_o**2)) / ys**2:.2e}")
    assert rel_err(mu, mu_o) < 1e-7
    assert np.max(np.abs(sd**2 - sd_o**2)) < 2e-5 * ys**2


def test_targets_only_append_recomputes_mu_and_rescales_sd(engine):
    c = Case(200, 5, 3000, 0, True, F.RBF)
    arm(engine, c)
    y2 = 3.0 * c.y[:c.N] + 0.5 * np.cos(c.X[:c.N].sum(1))            # other targets, another mean and std
    yn2, ym2, ys2 = O.normalize_targets(y2)
    assert abs(ys2 / c.norm(c.N)[2] - 1.0) > 0.5
    engine.fit_append(np.empty((0, c.d)), yn2)
    mu, sd, route = engine.posterior_refresh(0, ym2, ys2, return_route=True)
    assert route == 1
    mu_o, sd_o = c.truth(c.N, y2)
    print(f"{c.what} targets only: mu {rel_err(mu, mu_o):.2e} sd {rel_err(sd, sd_o):.2e}")
    S.check_posterior(mu, sd, mu_o, sd_o, ys2, c.what + " targets only", 1e-6)
    mu_f, sd_f = engine.posterior(0, ym2, ys2)
    S.check_posterior(mu, sd, mu_f, sd_f, ys2, c.what + " targets only vs full pass", 1e-6)


# ---- never stale ---------------------------------------------------------------------------------------------------------------
def _full_pass_expected(eng, ym, ys, what):
    mu, sd, route = eng.posterior_refresh(0, ym, ys, return_route=True)
    assert route == 0, f"after {what} the refresh must be the full pass"
    mu_f, sd_f = eng.posterior(0, ym, ys)
    assert np.array_equal(mu, mu_f) and np.array_equal(sd, sd_f), what
    assert np.isfinite(mu).all() and np.isfinite(sd).all()


def test_never_stale(engine):
    eng = engine
    c = Case(100, 3, 2000, 1, False, F.MATERN25)
    d, N = c.d, c.N
    yn, ym, ys = c.norm(N)
    rng = np.random.RandomState(11)
    other = rng.uniform(size=(1777, d))                        # other candidates, another count
    lo, hi = np.zeros(d), np.ones(d)
    groups = [(0, 0, d)]

    def eligible():
        arm(eng, c)
        append(eng, c, c.N0, N)

    # the armed state IS eligible (otherwise nothing below shows anything)
    eligible()
    assert eng.posterior_refresh(0, ym, ys, fetch=False, return_route=True)[2] == 1
    # a second refresh with nothing appended in between: the posterior is valid, not stale — the full pass
    _full_pass_expected(eng, ym, ys, "a refresh")

    # writers of the slot's fit
    def refit():
        eng.fit(c.X[:N], yn, c.kind, c.ls, NOISE)

    def fit_begin():
        with eng.overlapped_fits():
            eng.fit(c.X[:N], yn, c.kind, c.ls, NOISE)

    def fit_scaled():
        eng.fit(c.X[:N], yn, c.kind, c.ls, NOISE, amplitude=2.0, white=1e-3)

    def lml_then_fit():
        eng.lml(c.X[:N], yn, c.kind, c.ls, NOISE)
        with pytest.raises(GpboError, match="not been fitted"):       # gpbo_lml leaves the slot unfitted: STATE, as for every reader
            eng.posterior_refresh(0, ym, ys)
        eng.fit(c.X[:N], yn, c.kind, c.ls, NOISE)

    # writers of the candidates
    def set_candidates():
        eng.set_candidates(other)

    def generate_philox():
        eng.generate_candidates(1500, lo, hi, 12345)

    def generate_mt():
        eng.generate_candidates_like(1600, lo, hi, np.random.RandomState(4))

    def generate_trust_region():
        sv, shift = sobol_tables(d, 3)
        eng.generate_candidates_trust_region(1300, np.full(d, 0.4), lo, hi, sv, shift, 30, 2 ** 31, 0x1234567_89ABCDEF)

    def generate_columns_and_transform():
        eng.generate_candidates_mixed(1400, [(0, 0, d, lo, hi, None)], np.random.RandomState(5))
        eng.transform_candidates(groups)

    def predict():
        eng.predict(other[:300], 0, ym, ys)

    def predict_cov():
        eng.predict_cov(other[:200], 0, ym, ys)
        eng.n_candidates = 200

    def predict_grad():
        eng.predict_grad(other[:50], 0, ym, ys)

    def polish_seeds():
        eng.polish_seeds(O.UCB, 2.576, 0.0, None, None, [ym], [ys], other[:8], np.column_stack([lo, hi]), max_iter=3)
        eng.n_candidates = c.M          # the one-launch search left the context's candidates alone: they are still the M resident ones

    def evolve_mixed():
        eng.evolve_mixed(O.UCB, 2.576, 0.0, ym, ys, groups, np.column_stack([lo, hi]), other[:15], np.random.RandomState(6),
                         maxiter=2)

    for writer in (refit, fit_begin, fit_scaled, lml_then_fit, set_candidates, generate_philox, generate_mt,
                   generate_trust_region, generate_columns_and_transform, predict, predict_cov, predict_grad, polish_seeds, evolve_mixed):
        eligible()
        writer()
        _full_pass_expected(eng, ym, ys, writer.__name__)

    # a writer of the candidates BETWEEN the posterior and the append: the resident posterior was not valid for the current
    # candidates when the append ran
    arm(eng, c)
    eng.set_candidates(other)
    append(eng, c, c.N0, N)
    _full_pass_expected(eng, ym, ys, "set_candidates before the append")
    # an unfitted slot
    with pytest.raises(GpboError, match="not been fitted"):
        eng.posterior_refresh(5, ym, ys)
