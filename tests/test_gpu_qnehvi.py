"""GPU (-m gpu): gpbo_qnhvi_greedy — greedy batch noisy expected hypervolume improvement for two objectives over a resident
(2, T, M) block of posterior draws — against tests/qnehvi_truth.py.

Parity of the block and of the values at the base points: tests/test_gpu_sample_paths.py's norm (`err_of`) and bar — max(1e-9, 8 x
the spread between the two NumPy routes), or for the tiny case 8 x the fp64 restatement's own error against the 50-digit truth —
per objective.  Same bits as the plain draws: rows [g S, (g + 1) S) of objective j's block (and of its base values) are
gpbo_sample_paths' values_out for slot j and group g's inputs.
Fronts: fronts_out[0] is `front_of(base_values_out)` exactly, points, order and sizes.
Exact replay: the truth's greedy run ON THE DEVICE'S OWN values_out and fronts_out[0] reproduces keys_out bit for bit (-0.0 equal to
0.0), pick_idx / pick_gain and fronts_out[1] exactly — for every case with q = min(8, M), for q = M = 5 and for q = 64.  A key is a
sum of single rounded products in a fixed order: a wrong sum order, a contracted multiply-add, a stale front, an update from the
wrong column or a wrong LDS chunk shows here.
Picks against the independent truth: only the leading steps whose best and second-best key are at least GAP_FLOOR x (the first
step's gain) apart in the truth itself, at least two per case, asserted on the truth alone.
The shapes are the edges of the code: M = 1, odd and even (one or two candidates per score thread), several score workgroups and the
wide path_eval workgroup (M >= 2^17), T = 1, T = 10 (under the LDS stage of 16 draws) and T = 256 (16 stages), T = 48 (three), no
base point, slots that differ in N, kernel, scaling and precision, a slot after fit_append."""
import functools

import numpy as np
import pytest

import batch_truth as B
import matern_family_truth as F
import paths_truth as P
import qnehvi_truth as Q
from bayesianoptimization_amd import ParetoOptimizer, _lib, suggest_qnehvi
from bayesianoptimization_amd._lib import GpboError, dptr, iptr
from bayesianoptimization_amd.engine import F32, GpEngine, GroupEngine
from bayesianoptimization_amd.thompson import spectral_draw
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

NOISE = 1e-2
Y_MEAN, Y_STD = (3.5, -1.0), (0.4, 2.0)
BAR, MARGIN, GAP_FLOOR = 1e-9, 8.0, B.GAP_FLOOR
L = _lib.MAX_QNEHVI_FRONT

#: name -> (M, F, d, G, S, pending points, reference, seed, (slot 0, slot 1)), a slot = (N, kind, variant)
CASES = {
    "n1-m1-f1-d1-1x1-b0": (1, 1, 1, 1, 1, None, "mp", 0, ((1, F.RBF, "plain"), (1, F.RBF, "plain"))),
    "n65-m63-f64-d2-2x5-p1": (63, 64, 2, 2, 5, 1, "fp64", 0, ((65, F.MATERN25, "plain"), (65, F.MATERN25, "plain"))),
    "n64-m64-f63-d3-16x16-p0": (64, 63, 3, 16, 16, 0, "fp64", 0, ((64, F.RBF, "append"), (64, F.MATERN25, "plain"))),
    "n130+65-m257-f65-d5-3x16-p64": (257, 65, 5, 3, 16, 64, "fp64", 0, ((130, F.MATERN15, "scaled"), (65, F.RBF, "f32"))),
    "n65-m131075-f63-d2-2x1-p0": ((1 << 17) + 3, 63, 2, 2, 1, 0, "fp64", 0, ((65, F.MATERN25, "plain"), (65, F.RBF, "plain"))),
}
#: the cases whose leading picks are compared with the truth's (each needs two separated steps in the truth itself)
PICK_CASES = ["n65-m63-f64-d2-2x5-p1", "n130+65-m257-f65-d5-3x16-p64", "n64-m64-f63-d3-16x16-p0"]


def length_scale(d, j):
    s = (0.5, 0.7)[j] * np.sqrt(d)
    return s * np.geomspace(0.75, 1.33, d) if d > 1 else np.array([s])


def err_of(f, ref, j):
    ref_n = (ref - Y_MEAN[j]) / Y_STD[j]
    return float(np.max(np.abs(f - ref)) / (Y_STD[j] * max(1.0, float(np.max(np.abs(ref_n))))))


class Slot:
    def __init__(self, j, X, y, kind, variant, Fn, G, S, rs):
        self.j, self.X, self.kind, self.variant = j, X, kind, variant
        self.N, d = X.shape
        self.yn = (y - y.mean()) / y.std() if self.N > 1 else np.array([0.3 - 0.5 * j])
        self.ls = length_scale(d, j)
        self.amplitude, self.white = (2.5, 1e-3) if variant == "scaled" else (1.0, 0.0)
        self.eta = (NOISE + self.white) / self.amplitude
        self.groups = []
        for _ in range(G):
            omega, phase = spectral_draw(kind, Fn, d, rs)
            w = rs.standard_normal((S, Fn))
            self.groups.append((omega, phase, w, rs.standard_normal((S, self.N)) * np.sqrt(NOISE + self.white)))

    def route(self, fn, pts):
        return Q.group_values(fn, self.kind, self.X, self.yn, self.ls, self.eta, self.groups, pts, Y_MEAN[self.j], Y_STD[self.j],
                              self.amplitude)

    def fit(self, eng):
        j = self.j
        if self.variant == "append":           # other targets before the append: every target changes with it
            n0 = self.N - 3
            eng.fit(self.X[:n0], self.yn[:n0] * 1.1 - 0.05, self.kind, self.ls, NOISE, slot=j)
            eng.fit_append(self.X[n0:], self.yn, slot=j)
            return
        kw = {"amplitude": self.amplitude, "white": self.white} if self.variant == "scaled" else {}
        eng.fit(self.X, self.yn, self.kind, self.ls, NOISE, slot=j, precision=F32 if self.variant == "f32" else 0, **kw)


class Case:
    """Data, draws and references of one case (computed once, shared, never changed)."""

    def __init__(self, M, Fn, d, G, S, pending, reference, seed, slots):
        self.M, self.F, self.d, self.G, self.S, self.T, self.reference = M, Fn, d, G, S, G * S, reference
        N0 = max(s[0] for s in slots)
        X, y0 = F.data(N0, d, seed=seed + 17 * N0 + d)
        y1 = np.cos(3.0 * X.sum(1) + 0.7) + 0.1 * np.random.RandomState(seed + 5).standard_normal(N0)
        rs = np.random.RandomState(3000 + seed + N0 + M + Fn)
        self.Xc = rs.uniform(size=(M, d))
        self.slots = [Slot(j, X[:n], (y0, y1)[j][:n], kind, variant, Fn, G, S, rs) for j, (n, kind, variant) in enumerate(slots)]
        # base: the observed points (the larger slot's), then the pending ones; None: no base point at all
        self.base = None if pending is None else np.vstack([X, rs.uniform(size=(pending, d))])
        self.n_base = 0 if self.base is None else self.base.shape[0]
        # ref at the objectives' lower quartiles, raw units
        self.refp = np.array([Y_MEAN[j] + Y_STD[j] * float(np.quantile(s.yn, 0.25)) for j, s in enumerate(self.slots)])
        self.draws = [s.groups for s in self.slots]
        self.what = f"M={M} F={Fn} d={d} {G}x{S} B={self.n_base} " + " | ".join(f"N={s.N} kind {s.kind} {s.variant}" for s in self.slots)

    def route(self, fn):
        """(2, T, M + B): the draws at the candidates | the base points"""
        pts = self.Xc if self.base is None else np.vstack([self.Xc, self.base])
        return np.stack([s.route(fn, pts) for s in self.slots])

    def references(self):
        cho = self.route(P.paths_cho)
        other = self.route(P.paths_mp if self.reference == "mp" else P.paths_winv)
        ref = other if self.reference == "mp" else cho
        own = [err_of(cho[j], other[j], j) for j in range(2)]
        return ref, [max(BAR, MARGIN * o) for o in own], own

    def fit(self, eng):
        for s in self.slots:
            s.fit(eng)
        eng.set_candidates(self.Xc)

    def run(self, eng, q, draws=None, **kw):
        kw.setdefault("base", self.base)
        return eng.qnehvi_greedy(self.draws if draws is None else draws, q, self.refp, y_mean=Y_MEAN, y_std=Y_STD, return_values=True,
                                 return_keys=True, return_fronts=True, **kw)


@functools.lru_cache(maxsize=None)
def case_of(name):
    c = Case(*CASES[name])
    c.ref, c.bar, c.own = c.references()
    return c


def replay(c, out, q, what, index_offset=0):
    """fronts_out[0] is the front of base_values_out; the truth's greedy on the device's own values and fronts: keys bit for bit,
    picks, gains and fronts_out[1] exactly"""
    T = out["values"].shape[1]
    before, after = Q.unpack(out["front_size"][0], out["fronts"][0]), Q.unpack(out["front_size"][1], out["fronts"][1])
    built = Q.fronts_of(out["base_values"], c.refp) if out["base_values"].shape[2] else [np.empty((0, 2))] * T
    assert Q.same_fronts(before, built), f"{what}: fronts_out[0] is not the front of base_values_out"
    assert out["keys"].shape == (q, out["values"].shape[2]) and out["index"].shape == (q,) and out["gain"].shape == (q,)
    t_idx, t_gain, t_keys, t_fronts = Q.greedy(out["values"], before, c.refp, q, index_offset)
    keys = out["keys"]
    assert np.array_equal(keys, t_keys, equal_nan=True), f"{what}: keys differ at {np.argwhere(~((keys == t_keys) | (np.isnan(keys) & np.isnan(t_keys))))[:4].tolist()}"
    assert np.array_equal(out["index"], t_idx), f"{what}: picks {out['index'].tolist()}, replay {t_idx.tolist()}"
    assert np.array_equal(out["gain"], t_gain, equal_nan=True) and not np.signbit(out["gain"][out["gain"] == 0.0]).any()
    assert Q.same_fronts(after, t_fronts), f"{what}: fronts_out[1] is not the replay's"
    return t_idx, t_gain


# ---- parity, the fronts, the replay and the picks, case by case ----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_parity_fronts_and_exact_replay(engine, name):
    c = case_of(name)
    c.fit(engine)
    q = min(8, c.M)
    out = c.run(engine, q)
    assert out["values"].shape == (2, c.T, c.M) and out["base_values"].shape == (2, c.T, c.n_base)
    assert out["front_size"].shape == (2, c.T) and out["fronts"].shape == (2, c.T, L, 2)
    for j in range(2):
        e = err_of(out["values"][j], c.ref[j][:, :c.M], j)
        eb = err_of(out["base_values"][j], c.ref[j][:, c.M:], j) if c.n_base else 0.0
        print(f"{c.what}: objective {j}: values {e:.2e}, base values {eb:.2e}, bar {c.bar[j]:.2e} (the reference's own {c.own[j]:.2e})")
        assert e <= c.bar[j] and eb <= c.bar[j], f"{c.what}: objective {j}: error {e:.2e} / {eb:.2e} over its bar {c.bar[j]:.2e}"
    replay(c, out, q, c.what)
    sizes = out["front_size"]
    print(f"{c.what}: fronts of {sizes[0].min()}..{sizes[0].max()} points before, {sizes[1].min()}..{sizes[1].max()} after")
    if c.n_base == 0:
        assert (sizes[0] == 0).all()
    else:
        assert sizes[0].max() >= 2 and sizes.max() < L


@pytest.mark.parametrize("name", PICK_CASES)
def test_leading_picks_against_the_truth(engine, name):
    c = case_of(name)
    q = 8
    f0 = Q.fronts_of(c.ref[:, :, c.M:], c.refp)
    t_idx, t_gain, t_keys, _ = Q.greedy(c.ref[:, :, :c.M], f0, c.refp, q)
    n, gaps = Q.leading_separated_steps(t_keys, GAP_FLOOR)
    print(f"{c.what}: truth picks {t_idx.tolist()}, gaps {['%.1e' % g for g in gaps]}: {n} leading separated steps")
    assert n >= 2, f"{c.what}: only {n} separated leading steps in the truth itself: pick another seed"
    c.fit(engine)
    out = c.run(engine, q)
    assert np.array_equal(out["index"][:n], t_idx[:n]), f"{c.what}: picks {out['index'][:n].tolist()}, truth {t_idx[:n].tolist()}"
    # a gain is a mean of areas between two monotone staircases inside (W, H) = the values' spans above ref: moving every corner by
    # (e_0, e_1), the values' bars in raw units, moves an area by at most 2 (e_0 H + e_1 W) to first order; twice that is allowed
    e = [c.bar[j] * Y_STD[j] * max(1.0, float(np.abs((c.ref[j] - Y_MEAN[j]) / Y_STD[j]).max())) for j in range(2)]
    W, H = (float(c.ref[j].max() - c.refp[j]) for j in range(2))
    assert np.allclose(out["gain"][:n], t_gain[:n], rtol=0.0, atol=4.0 * (e[0] * H + e[1] * W))


def test_same_bits_as_the_plain_draws(engine):
    c = case_of("n130+65-m257-f65-d5-3x16-p64")
    c.fit(engine)
    out = c.run(engine, 2)
    for j, s in enumerate(c.slots):
        for g, (omega, phase, w, eps) in enumerate(s.groups):
            engine.set_candidates(c.Xc)
            _, _, plain = engine.sample_paths(omega, phase, w, eps, slot=j, y_mean=Y_MEAN[j], y_std=Y_STD[j], return_values=True)
            assert np.array_equal(out["values"][j, g * c.S:(g + 1) * c.S], plain), f"objective {j} group {g}: not gpbo_sample_paths' values"
            engine.set_candidates(c.base)
            _, _, plain = engine.sample_paths(omega, phase, w, eps, slot=j, y_mean=Y_MEAN[j], y_std=Y_STD[j], return_values=True)
            assert np.array_equal(out["base_values"][j, g * c.S:(g + 1) * c.S], plain), f"objective {j} group {g}: base values"


# ---- the exact replay at the other batch sizes --------------------------------------------------------------------------------------
def test_replay_q_equals_m_and_q_64(engine):
    c = case_of("n65-m63-f64-d2-2x5-p1")
    c.fit(engine)
    engine.set_candidates(c.Xc[:5])
    idx, gain = replay(c, c.run(engine, 5), 5, "q = M = 5")
    assert sorted(idx.tolist()) == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError, match="q exceeds"):
        c.run(engine, 6)
    # q = 64, the most: M = 64 (even: two candidates per thread), then M = 257 (odd)
    engine.set_candidates(np.vstack([c.Xc, c.Xc[:1] * 0.5]))
    idx, _ = replay(c, c.run(engine, 64), 64, "q = M = 64")
    assert sorted(idx.tolist()) == list(range(64))
    big = case_of("n130+65-m257-f65-d5-3x16-p64")
    big.fit(engine)
    idx, gain = replay(big, big.run(engine, 64), 64, "q = 64 of 257")
    assert len(set(idx.tolist())) == 64 and gain[0] > 0.0


# ---- the front build and the update rule on raw values ------------------------------------------------------------------------------
def _debug_fronts(eng, pairs_per_draw, ref, inserts=None):
    """the device's fronts of per-draw pair lists (all of one length), as a list of (n, 2) arrays"""
    bv = np.ascontiguousarray(np.stack([np.array(p, dtype=np.float64).reshape(-1, 2).T for p in pairs_per_draw], axis=1))
    iv = None if inserts is None else np.ascontiguousarray(np.stack([np.array(p, dtype=np.float64).reshape(-1, 2).T for p in inserts], axis=1))
    size, fronts = eng.debug_qnehvi_fronts(bv, ref, iv)
    return Q.unpack(size, fronts)


def test_fronts_on_raw_values(debug_engine):
    eng = debug_engine
    nan = np.nan
    ref = np.array([0.0, 0.0])
    # duplicates, ties in one objective, points on ref, NaNs — and a draw wholly below ref
    a = [[1.0, 1.0], [2.0, 0.5], [2.0, 0.5], [0.5, 3.0], [1.0, 0.9], [nan, 9.0], [9.0, nan], [0.0, 5.0], [5.0, 0.0], [2.0, 0.4], [0.5, 2.0],
         [1.0, 1.0]]
    b = [[-1.0, -2.0]] * 6 + [[0.0, 0.0], [-0.0, 3.0], [3.0, -1.0], [nan, nan], [-5.0, 5.0], [0.0, 1.0]]
    got = _debug_fronts(eng, [a, b], ref)
    assert got[0].tolist() == [[2.0, 0.5], [1.0, 1.0], [0.5, 3.0]] and got[1].shape == (0, 2)
    assert Q.same_fronts(got, [Q.front_of(a, ref), Q.front_of(b, ref)])
    # n = 0, and n = 1025 random pairs on a coarse grid (several elements per thread, a ragged last round), 300 draws
    size, _ = eng.debug_qnehvi_fronts(np.empty((2, 3, 0)), ref)
    assert size.tolist() == [0, 0, 0]
    rs = np.random.RandomState(0)
    bv = np.round(rs.standard_normal((2, 300, 1025)), 1)
    bv[rs.uniform(size=bv.shape) < 0.01] = nan
    size, fronts = eng.debug_qnehvi_fronts(bv, [-0.5, 0.25])
    assert Q.same_fronts(Q.unpack(size, fronts), Q.fronts_of(bv, [-0.5, 0.25])) and size.max() >= 4
    # the update rule, in order, against the truth's
    ins = np.round(rs.standard_normal((2, 300, 9)), 1)
    ins[0, :, 3] = nan
    size, fronts = eng.debug_qnehvi_fronts(bv, [-0.5, 0.25], ins)
    want = Q.fronts_of(bv, [-0.5, 0.25])
    for i in range(9):
        want = [Q.insert(f, ins[:, t, i], [-0.5, 0.25]) for t, f in enumerate(want)]
    assert Q.same_fronts(Q.unpack(size, fronts), want)
    # an anti-diagonal of exactly 128 non-dominated points passes (given in ascending order, among dominated ones); 129 are refused
    diag = lambda n: [[float(k), float(n + 1 - k)] for k in range(1, n + 1)]
    full = np.array(diag(128)[::-1])
    got = _debug_fronts(eng, [diag(128) + [[0.5, 0.5]], diag(128)[::-1] + [[1.0, 1.0]]], ref)
    assert np.array_equal(got[0], full) and np.array_equal(got[1], full)
    with pytest.raises(NotImplementedError, match="draw 1 outgrew 128"):
        _debug_fronts(eng, [diag(128) + [[0.5, 0.5]], diag(129)], ref)
    # ... and a call after a refusal works
    assert np.array_equal(_debug_fronts(eng, [diag(128)], ref)[0], full)
    # an insertion into a full front that dominates three points passes at 126; one that dominates none is refused
    got = _debug_fronts(eng, [diag(128)], ref, [[[5.5, 126.5]]])
    assert got[0].shape == (126, 2) and np.array_equal(got[0], Q.insert(full, [5.5, 126.5], ref))
    with pytest.raises(NotImplementedError, match="draw 0 outgrew 128"):
        _debug_fronts(eng, [diag(128)], ref, [[[0.5, 200.0]]])
    got = _debug_fronts(eng, [diag(128)], ref, [[[0.5, 100.0], [128.0, 1.0], [nan, 500.0], [0.0, 500.0]]])      # dominated, equal, NaN, on ref
    assert np.array_equal(got[0], full)


# ---- conventions ------------------------------------------------------------------------------------------------------------------
def test_nan_offset_repeatable_and_leaks(engine):
    c = case_of("n65-m63-f64-d2-2x5-p1")
    c.fit(engine)
    base = c.run(engine, 6)
    again = c.run(engine, 6)
    for k in base:                                                   # bitwise repeatable
        assert np.array_equal(base[k], again[k], equal_nan=True), k
    off = c.run(engine, 6, index_offset=10**10)
    assert np.array_equal(off["index"], base["index"] + 10**10) and np.array_equal(off["gain"], base["gain"])
    replay(c, off, 6, "index_offset", index_offset=10**10)
    # a call after qnei_greedy / sample_paths on either slot, and one before them, leaks nothing
    g0 = c.slots[0].groups
    qnei = engine.qnei_greedy(g0, 3, y_mean=Y_MEAN[0], y_std=Y_STD[0], return_values=True, return_keys=True)
    plain = engine.sample_paths(*c.slots[1].groups[0], slot=1, y_mean=Y_MEAN[1], y_std=Y_STD[1], return_values=True)
    after = c.run(engine, 6)
    for k in base:
        assert np.array_equal(base[k], after[k], equal_nan=True), k
    qnei2 = engine.qnei_greedy(g0, 3, y_mean=Y_MEAN[0], y_std=Y_STD[0], return_values=True, return_keys=True)
    plain2 = engine.sample_paths(*c.slots[1].groups[0], slot=1, y_mean=Y_MEAN[1], y_std=Y_STD[1], return_values=True)
    assert all(np.array_equal(a, b) for a, b in zip(qnei, qnei2)) and all(np.array_equal(a, b) for a, b in zip(plain, plain2))
    # no base point: every front starts empty
    none = c.run(engine, 4, base=None)
    assert (none["front_size"][0] == 0).all() and np.array_equal(none["values"], base["values"])
    replay(c, none, 4, "no base")
    # a NaN candidate: its key is NaN, it wins step 0 with gain NaN, is masked from step 1 on, and leaves every front as it was
    k = next(i for i in range(c.M - 1, -1, -1) if i not in base["index"][:3])
    Xn = c.Xc.copy()
    Xn[k, 1] = np.nan
    engine.set_candidates(Xn)
    out = c.run(engine, 4)
    assert out["index"][0] == k and np.isnan(out["gain"][0]) and np.isfinite(out["gain"][1:]).all() and out["keys"][1][k] == np.inf
    assert np.array_equal(out["index"][1:], base["index"][:3]) and np.array_equal(out["gain"][1:], base["gain"][:3])
    replay(c, out, 4, "a NaN candidate")


# ---- a reader ------------------------------------------------------------------------------------------------------------------------
def test_reader_only(engine):
    eng = engine
    c = case_of("n65-m63-f64-d2-2x5-p1")
    c.fit(eng)
    alpha = [eng.get_alpha(c.slots[j].N, slot=j) for j in range(2)]
    post = [eng.posterior(j, Y_MEAN[j], Y_STD[j]) for j in range(2)]
    eng.take_negative_variance_flag()
    before = eng.acq_argbest(O.UCB, 2.576, k_seeds=8, return_values=True)
    c.run(eng, 8)
    after = eng.acq_argbest(O.UCB, 2.576, k_seeds=8, return_values=True)      # still answers, from the posterior before the call
    assert before[0] == after[0] and before[1] == after[1] and all(np.array_equal(a, b) for a, b in zip(before[2:], after[2:]))
    assert all(np.array_equal(eng.get_alpha(c.slots[j].N, slot=j), alpha[j]) for j in range(2))
    assert np.array_equal(eng.get_candidate_rows(np.arange(c.M), c.d), c.Xc)
    assert eng.take_negative_variance_flag() is False
    for j in range(2):
        mu, sd = eng.posterior(j, Y_MEAN[j], Y_STD[j])
        assert np.array_equal(mu, post[j][0]) and np.array_equal(sd, post[j][1])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(engine):
    eng = engine
    c = case_of("n65-m63-f64-d2-2x5-p1")
    c.fit(eng)
    G, S, Fn, d = c.G, c.S, c.F, c.d
    flat = [g for s in c.slots for g in s.groups]
    omega = np.ascontiguousarray(np.concatenate([g[0].ravel() for g in flat]))
    phase = np.ascontiguousarray(np.concatenate([g[1] for g in flat]))
    w = np.ascontiguousarray(np.concatenate([g[2].ravel() for g in flat]))
    eps = np.ascontiguousarray(np.concatenate([g[3].ravel() for g in flat]))
    base = np.ascontiguousarray(c.base)
    pi, pg = np.empty(64, dtype=np.int64), np.empty(64)
    arr = lambda v: np.ascontiguousarray(np.array(v, dtype=np.float64))
    keep = []

    def call(h=None, y_mean=Y_MEAN, y_std=Y_STD, n_groups=G, n_paths=S, n_features=Fn, draws=None, ref=c.refp, base_p=dptr(base),
             n_base=c.n_base, dd=d, q=4, outs=None):
        draws = [dptr(omega), dptr(phase), dptr(w), dptr(eps)] if draws is None else draws
        outs = [iptr(pi), dptr(pg)] if outs is None else outs
        ym, ys, rf = (None if v is None else arr(v) for v in (y_mean, y_std, ref))
        keep[:] = [ym, ys, rf]
        return eng._lib.gpbo_qnhvi_greedy(eng._h if h is None else h, dptr(ym), dptr(ys), n_groups, n_paths, n_features, *draws,
                                           dptr(rf), base_p, n_base, dd, q, 0, *outs, None, None, None, None, None)

    assert call() == _lib.GPBO_OK
    assert call(n_groups=0) == _lib.ERR_INVALID and call(n_groups=17) == _lib.ERR_INVALID
    assert call(n_paths=0) == _lib.ERR_INVALID and call(n_paths=17) == _lib.ERR_INVALID
    assert call(n_features=0) == _lib.ERR_INVALID and call(n_features=4097) == _lib.ERR_INVALID
    # a NULL among the inputs, ref, pick_idx or pick_gain
    for k in range(4):
        a = [dptr(omega), dptr(phase), dptr(w), dptr(eps)]
        a[k] = None
        assert call(draws=a) == _lib.ERR_INVALID
    for k in range(2):
        a = [iptr(pi), dptr(pg)]
        a[k] = None
        assert call(outs=a) == _lib.ERR_INVALID
    assert call(ref=None) == _lib.ERR_INVALID and call(y_mean=None) == _lib.ERR_INVALID and call(y_std=None) == _lib.ERR_INVALID
    # a y_std not finite or not positive, a y_mean or ref not finite — in either objective
    for j in range(2):
        for bad in (0.0, -1.0, np.inf, np.nan):
            v = list(Y_STD)
            v[j] = bad
            assert call(y_std=v) == _lib.ERR_INVALID
        for bad in (np.inf, -np.inf, np.nan):
            v, r = list(Y_MEAN), list(c.refp)
            v[j], r[j] = bad, bad
            assert call(y_mean=v) == _lib.ERR_INVALID and call(ref=r) == _lib.ERR_INVALID
    # n_base outside [0, GPBO_MAX_QNEHVI_BASE], n_base > 0 with a NULL or non-finite base, d not the slots'
    assert call(n_base=-1) == _lib.ERR_INVALID and call(n_base=_lib.MAX_QNEHVI_BASE + 1) == _lib.ERR_INVALID
    assert call(base_p=None, n_base=1) == _lib.ERR_INVALID and call(base_p=None, n_base=0) == _lib.GPBO_OK
    for bad in (np.nan, np.inf):
        pb = base.copy()
        pb[-1, 1] = bad
        assert call(base_p=dptr(pb)) == _lib.ERR_INVALID
    assert call(dd=d + 1) == _lib.ERR_INVALID and call(dd=d + 1, base_p=None, n_base=0) == _lib.ERR_INVALID
    # q outside [1, GPBO_MAX_SEEDS], or q > M
    assert call(q=0) == _lib.ERR_INVALID and call(q=65) == _lib.ERR_INVALID
    assert call(q=63) == _lib.GPBO_OK and call(q=64) == _lib.ERR_INVALID             # M = 63
    # the engine's own refusals, as exceptions
    with pytest.raises(ValueError, match="two lists"):
        eng.qnehvi_greedy([c.draws[0]], 2, c.refp)
    with pytest.raises(ValueError, match="n_groups"):
        eng.qnehvi_greedy([c.draws[0] * 9, c.draws[1] * 9], 2, c.refp)
    with pytest.raises(ValueError, match="same non-empty list"):
        eng.qnehvi_greedy([c.draws[0], c.draws[1][:1]], 2, c.refp)
    with pytest.raises(ValueError, match="base"):
        eng.qnehvi_greedy(c.draws, 2, c.refp, base=np.zeros((1, d + 1)))
    with pytest.raises(ValueError, match="q out of range"):
        eng.qnehvi_greedy(c.draws, 65, c.refp)
    # GPBO_ERR_STATE: a fit pending on slot 1 (asked at the C boundary), then slot 1 left unfitted by gpbo_lml
    s1 = c.slots[1]
    with eng.overlapped_fits():
        eng.fit(s1.X, s1.yn, s1.kind, s1.ls, NOISE, slot=1)
        assert call() == _lib.ERR_STATE
    assert call() == _lib.GPBO_OK
    eng.lml(s1.X, s1.yn, s1.kind, s1.ls, NOISE, slot=1)
    assert call() == _lib.ERR_STATE
    with pytest.raises(GpboError, match="not been fitted"):
        eng.qnehvi_greedy(c.draws, 2, c.refp)
    # ... a slot of another d
    eng.fit(np.hstack([s1.X, s1.X[:, :1]]), s1.yn, s1.kind, np.array([1.0]), NOISE, slot=1)
    assert call() == _lib.ERR_STATE
    c.fit(eng)
    # ... candidates of another d
    eng.set_candidates(np.random.RandomState(1).uniform(size=(10, d + 1)))
    with pytest.raises(GpboError, match="dimension"):
        eng.qnehvi_greedy(c.draws, 2, c.refp, y_mean=Y_MEAN, y_std=Y_STD)
    # ... no resident candidates: a context that never had any
    fresh = GpEngine(0)
    try:
        assert call(h=fresh._h) == _lib.ERR_STATE
        for s in c.slots:
            s.fit(fresh)
        with pytest.raises(GpboError, match="no candidates"):
            fresh.qnehvi_greedy(c.draws, 2, c.refp, y_mean=Y_MEAN, y_std=Y_STD)
    finally:
        fresh.close()
    # a device group
    with pytest.raises(NotImplementedError, match="device group"):
        GroupEngine.qnehvi_greedy(object.__new__(GroupEngine), c.draws, 2, c.refp)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def test_suggest_qnehvi_end_to_end(engine):
    bounds = {"a": (0.0, 1.0), "b": (-1.0, 2.0), "c": (0.5, 1.5)}
    lo, hi = np.array(list(bounds.values())).T
    X = lo + np.random.RandomState(0).uniform(size=(30, 3)) * (hi - lo)
    noise = 0.05 * np.random.RandomState(1).standard_normal((30, 2))
    Y = np.column_stack([np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1]) + X[:, 2] ** 2, -((X[:, 0] - 0.7) ** 2) - 0.3 * X[:, 1] + 0.2 * X[:, 2]]) + noise

    def run():
        opt = ParetoOptimizer(bounds, 2, [-1.5, -1.5], n_restarts_optimizer=2, random_state=11, engine=engine, alpha=1e-3)
        for x, y in zip(X, Y):
            opt.register(x, y)
        return opt, suggest_qnehvi(opt, 4, n_random=257, n_draws=20, n_features=128, pending=[dict(zip(bounds, X[0] * 0.5 + 0.3))],
                                   return_info=True)

    opt, (picks, info) = run()
    rows = np.array([[p[k] for k in bounds] for p in picks])
    assert rows.shape == (4, 3) and (rows >= lo).all() and (rows <= hi).all() and len({tuple(r) for r in rows}) == 4
    assert info["n_draws"] == 20 and info["gain"][0] > 0.0 and len(set(info["index"].tolist())) == 4
    assert 1 <= info["front_size_before"] < L and 1 <= info["front_size_after"] < L
    Xc = engine.get_candidate_rows(np.arange(257), 3)                         # the one candidate draw is still resident
    assert np.array_equal(rows, Xc[info["index"]])
    _, (picks2, info2) = run()
    assert picks2 == picks and np.array_equal(info2["gain"], info["gain"]) and np.array_equal(info2["index"], info["index"])
    # the models answer for the real data afterwards
    assert all(gp.X_train_.shape[0] == 30 for gp in opt._gps)
