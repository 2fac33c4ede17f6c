"""GPU (-m gpu): gpbo_qnei_greedy — greedy batch noisy expected improvement over a resident (T, M) block of posterior draws —
against tests/qnei_truth.py.

Parity of the block and the baselines: tests/test_gpu_sample_paths.py's norm (`err_of`) and bar — max(1e-9, 8 x the spread
between the two NumPy routes), or for the tiny cases 8 x the fp64 restatement's own error against the 50-digit truth; a baseline is
a maximum of such values, so its error is bounded by theirs and it is held to the same bar.
Same bits as the plain draws: rows [g S, (g + 1) S) of values_out are gpbo_sample_paths' values_out for group g's inputs.
Exact replay: the truth's greedy run ON THE DEVICE'S OWN values_out and baseline_out reproduces keys_out bit for bit (-0.0 equal
to 0.0) and pick_idx / pick_gain exactly — for every case with q = min(8, M), for q = M = 5 (every candidate once, ascending
through the zero-gain tail) and for q = 64.  No product enters a key, so NumPy's adds and its one division are the device's: a
wrong sum order, a wrong mask, a stale m_t or an update from the wrong column shows here.
Picks against the truth: only the leading steps whose best and second-best key are at least GAP_FLOOR of the value range apart
in the truth itself, at least two per case, asserted on the truth alone.
The shapes (N, M, F, d, G x S, P) are the edges of the code: M odd and even (one or two candidates per score thread), one and
several score workgroups, the wide path_eval workgroup (M >= 2^17), T = 1 and T = 256, 0 / 1 / 64 pending points, the LDS stage of
64 training points / features on both sides; between them all four kernel kinds, a scaled slot, an F32 slot, a slot after
fit_append."""
import functools

import numpy as np
import pytest

import batch_truth as B
import matern_family_truth as F
import paths_truth as P
import qnei_truth as Q
from bayesianoptimization_amd import _lib
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd import suggest_qnei
from bayesianoptimization_amd._lib import GpboError, dptr, iptr
from bayesianoptimization_amd.engine import F32, GpEngine, GroupEngine
from bayesianoptimization_amd.qnei import draw_layout
from bayesianoptimization_amd.thompson import spectral_draw
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

KNAME = {F.RBF: "rbf", F.MATERN25: "matern25", F.MATERN15: "matern15", F.MATERN05: "matern05"}
NOISE = 1e-2
Y_MEAN, Y_STD = 3.5, 0.4
BAR, MARGIN, GAP_FLOOR = 1e-9, 8.0, B.GAP_FLOOR

#: name -> (N, M, F, d, G, S, P, kind, one length scale per dimension, reference, slot variant, seed)
CASES = {
    "n1-m1-f1-d1-1x1-p0": (1, 1, 1, 1, 1, 1, 0, F.RBF, False, "mp", "plain", 0),
    "n65-m63-f64-d2-2x5-p1": (65, 63, 64, 2, 2, 5, 1, F.MATERN25, True, "mp", "plain", 0),
    "n64-m63-f63-d3-16x16-p0": (64, 63, 63, 3, 16, 16, 0, F.RBF, True, "fp64", "append", 4),      # (seed 4: two separated steps in the truth)
    "n130-m257-f65-d5-3x16-p64": (130, 257, 65, 5, 3, 16, 64, F.MATERN15, True, "fp64", "scaled", 0),
    "n800-m63-f64-d17-2x4-p3": (800, 63, 64, 17, 2, 4, 3, F.MATERN05, True, "fp64", "f32", 0),
    "n65-m131075-f63-d2-2x1-p0": (65, (1 << 17) + 3, 63, 2, 2, 1, 0, F.MATERN25, True, "fp64", "plain", 0),
}
#: the cases whose leading picks are compared with the truth's (each needs two separated steps in the truth itself)
PICK_CASES = ["n65-m63-f64-d2-2x5-p1", "n130-m257-f65-d5-3x16-p64", "n64-m63-f63-d3-16x16-p0"]


def length_scale(d, per_dim):
    s = 0.5 * np.sqrt(d)
    return s * np.geomspace(0.75, 1.33, d) if per_dim else np.array([s])


def err_of(f, ref):
    ref_n = (ref - Y_MEAN) / Y_STD
    return float(np.max(np.abs(f - ref)) / (Y_STD * max(1.0, float(np.max(np.abs(ref_n))))))


class Case:
    """Data, draws and references of one case (computed once, shared, never changed)."""

    def __init__(self, N, M, Fn, d, G, S, P_, kind, per_dim, reference, variant="plain", seed=0):
        self.N, self.M, self.F, self.d, self.G, self.S, self.P, self.kind = N, M, Fn, d, G, S, P_, kind
        self.T, self.reference, self.variant = G * S, reference, variant
        self.amplitude, self.white = (2.5, 1e-3) if variant == "scaled" else (1.0, 0.0)
        self.X, y = F.data(N, d, seed=seed + 17 * N + d)
        self.yn = (y - y.mean()) / y.std() if N > 1 else np.array([0.3])
        self.ls = length_scale(d, per_dim)
        rs = np.random.RandomState(2000 + seed + N + M + Fn)
        self.Xc = rs.uniform(size=(M, d))
        self.pending = rs.uniform(size=(P_, d)) if P_ else None
        self.groups = []
        for _ in range(G):
            omega, phase = spectral_draw(kind, Fn, d, rs)
            w = rs.standard_normal((S, Fn))
            self.groups.append((omega, phase, w, rs.standard_normal((S, N)) * np.sqrt(NOISE + self.white)))
        self.eta = (NOISE + self.white) / self.amplitude
        self.what = f"N={N} M={M} F={Fn} d={d} {G}x{S} P={P_} {KNAME[kind]} {variant}"

    def route(self, fn):
        """(T, M + N + P): the draws at the candidates | the training points | the pending points"""
        pts = np.vstack([self.Xc, self.X] + ([self.pending] if self.P else []))
        return Q.group_values(fn, self.kind, self.X, self.yn, self.ls, self.eta, self.groups, pts, Y_MEAN, Y_STD, self.amplitude)

    def references(self):
        cho = self.route(P.paths_cho)
        if self.reference == "mp":
            ref = self.route(P.paths_mp)
            own = err_of(cho, ref)
        else:
            ref = cho
            own = err_of(self.route(P.paths_winv), cho)
        return ref, max(BAR, MARGIN * own), own

    def split(self, all_values):
        M, N = self.M, self.N
        return all_values[:, :M], all_values[:, M:M + N], (all_values[:, M + N:] if self.P else None)

    def fit(self, eng):
        if self.variant == "append":           # other targets before the append: every target changes with it
            n0 = self.N - 3
            eng.fit(self.X[:n0], self.yn[:n0] * 1.1 - 0.05, self.kind, self.ls, NOISE)
            eng.set_candidates(self.Xc)
            eng.fit_append(self.X[n0:], self.yn)
            return
        kw = {"amplitude": self.amplitude, "white": self.white} if self.variant == "scaled" else {}
        eng.fit(self.X, self.yn, self.kind, self.ls, NOISE, precision=F32 if self.variant == "f32" else 0, **kw)
        eng.set_candidates(self.Xc)

    def run(self, eng, q, groups=None, **kw):
        kw.setdefault("pending", self.pending)
        return eng.qnei_greedy(self.groups if groups is None else groups, q, y_mean=Y_MEAN, y_std=Y_STD, return_values=True,
                               return_keys=True, **kw)


@functools.lru_cache(maxsize=None)
def case_of(name):
    c = Case(*CASES[name])
    c.ref, c.bar, c.own = c.references()
    return c


def replay(c, out, q, what, index_offset=0):
    """the truth's greedy on the device's own values and baselines: keys bit for bit, picks and gains exactly"""
    idx, gain, m0, values, keys = out
    assert values.shape[1] == keys.shape[1] and keys.shape[0] == q and idx.shape == (q,) and gain.shape == (q,)
    t_idx, t_gain, t_keys, _ = Q.greedy(values, m0, q, index_offset)
    assert np.array_equal(keys, t_keys, equal_nan=True), f"{what}: keys differ at {np.argwhere(~((keys == t_keys) | (np.isnan(keys) & np.isnan(t_keys))))[:4].tolist()}"
    assert np.array_equal(idx, t_idx), f"{what}: picks {idx.tolist()}, replay {t_idx.tolist()}"
    assert np.array_equal(gain, t_gain, equal_nan=True) and not np.signbit(gain[gain == 0.0]).any()
    return t_idx, t_gain


# ---- parity, the replay and the picks, case by case ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_parity_and_exact_replay(engine, name):
    c = case_of(name)
    c.fit(engine)
    q = min(8, c.M)
    out = c.run(engine, q)
    idx, gain, m0, values, keys = out
    assert values.shape == (c.T, c.M) and m0.shape == (c.T,)
    ref_c, ref_x, ref_p = c.split(c.ref)
    e = err_of(values, ref_c)
    want_m = Q.baseline(ref_x, ref_p)
    em = err_of(m0, want_m)
    print(f"{c.what}: values {e:.2e}, baselines {em:.2e}, bar {c.bar:.2e} (the reference's own {c.own:.2e})")
    assert e <= c.bar, f"{c.what}: error {e:.2e} over its bar {c.bar:.2e}"
    assert em <= c.bar, f"{c.what}: baseline error {em:.2e} over its bar {c.bar:.2e}"
    replay(c, out, q, c.what)
    # noisy = 0: y_best and the pending points alone
    out0 = c.run(engine, q, noisy=False, y_best=float(np.median(ref_c)))
    assert np.array_equal(out0[3], values)
    em0 = err_of(out0[2], Q.baseline(ref_x, ref_p, noisy=False, y_best=float(np.median(ref_c))))
    assert em0 <= c.bar and (c.P or np.array_equal(out0[2], np.full(c.T, float(np.median(ref_c)))))
    replay(c, out0, q, c.what + " noisy=0")


@pytest.mark.parametrize("name", PICK_CASES)
def test_leading_picks_against_the_truth(engine, name):
    c = case_of(name)
    ref_c, ref_x, ref_p = c.split(c.ref)
    q = 8
    t_idx, t_gain, t_keys, _ = Q.greedy(ref_c, Q.baseline(ref_x, ref_p), q)
    n, gaps = Q.leading_separated_steps(ref_c, t_keys, GAP_FLOOR)
    print(f"{c.what}: truth picks {t_idx.tolist()}, gaps {['%.1e' % g for g in gaps]}: {n} leading separated steps")
    assert n >= 2, f"{c.what}: only {n} separated leading steps in the truth itself: pick another seed"
    c.fit(engine)
    idx, gain, _, _, _ = c.run(engine, q)
    assert np.array_equal(idx[:n], t_idx[:n]), f"{c.what}: picks {idx[:n].tolist()}, truth {t_idx[:n].tolist()}"
    assert np.allclose(gain[:n], t_gain[:n], rtol=0.0, atol=c.bar * Y_STD * max(1.0, np.abs((ref_c - Y_MEAN) / Y_STD).max()) * 2)


def test_same_bits_as_the_plain_draws(engine):
    c = case_of("n130-m257-f65-d5-3x16-p64")
    c.fit(engine)
    _, _, _, values, _ = c.run(engine, 2)
    for g, (omega, phase, w, eps) in enumerate(c.groups):
        _, _, plain = engine.sample_paths(omega, phase, w, eps, y_mean=Y_MEAN, y_std=Y_STD, return_values=True)
        assert np.array_equal(values[g * c.S:(g + 1) * c.S], plain), f"group {g}: the block's rows are not gpbo_sample_paths' values"
    # one draw, no noise model, an incumbent below every value: the first pick is the draw's maximiser
    omega, phase, w, eps = c.groups[1]
    for s in (0, 7, 15):
        one = [(omega, phase, w[s:s + 1], eps[s:s + 1])]
        best_idx, best_val, plain = engine.sample_paths(*one[0], y_mean=Y_MEAN, y_std=Y_STD, return_values=True)
        idx, gain, m0, vals, _ = c.run(engine, 1, groups=one, noisy=False, y_best=float(plain.min()) - 1.0, pending=None)
        assert np.array_equal(vals, plain) and idx[0] == best_idx[0] and m0[0] == float(plain.min()) - 1.0
        assert gain[0] == (0.0 + (best_val[0] - m0[0])) / 1.0


# ---- the exact replay at the other batch sizes ------------------------------------------------------------------------------------------
def test_replay_q_equals_m_and_q_64(engine):
    c = case_of("n65-m63-f64-d2-2x5-p1")
    c.fit(engine)
    # q = M = 5: every candidate once, ascending through the zero-gain tail
    engine.set_candidates(c.Xc[:5])
    out = c.run(engine, 5)
    idx, gain = replay(c, out, 5, "q = M = 5")
    assert sorted(idx.tolist()) == [0, 1, 2, 3, 4]
    zero = gain == 0.0
    assert zero.any() and (np.diff(idx[zero]) > 0).all() and (gain[~zero] > 0.0).all()
    with pytest.raises(ValueError, match="q exceeds"):
        c.run(engine, 6)
    # q = 64, the most: M = 64 (even: two candidates per thread), then M = 257 (odd)
    engine.set_candidates(np.vstack([c.Xc, c.Xc[:1] * 0.5]))
    idx, _ = replay(c, c.run(engine, 64), 64, "q = M = 64")
    assert sorted(idx.tolist()) == list(range(64))
    big = case_of("n130-m257-f65-d5-3x16-p64")
    big.fit(engine)
    idx, gain = replay(big, big.run(engine, 64), 64, "q = 64 of 257")
    assert len(set(idx.tolist())) == 64 and (np.diff(gain) <= 0.0).all()


# ---- conventions ---------------------------------------------------------------------------------------------------------------------
def test_nan_ties_offset_repeatable_and_grouping(engine):
    c = case_of("n65-m63-f64-d2-2x5-p1")
    c.fit(engine)
    base = c.run(engine, 6)
    again = c.run(engine, 6)
    for a, b in zip(base, again):                                   # bitwise repeatable
        assert np.array_equal(a, b, equal_nan=True)
    # index_offset is added, nothing else changes
    off = c.run(engine, 6, index_offset=10**10)
    assert np.array_equal(off[0], base[0] + 10**10) and np.array_equal(off[1], base[1]) and np.array_equal(off[4], base[4])
    replay(c, off, 6, "index_offset", index_offset=10**10)
    # T draws as one group or as part of more groups: the same rows, the same incumbents
    one = c.run(engine, 3, groups=c.groups[1:])
    assert np.array_equal(one[3], base[3][c.S:]) and np.array_equal(one[2], base[2][c.S:])
    replay(c, one, 3, "the second group alone")
    # a NaN planted through one weight: that draw is NaN everywhere, every key is NaN, the first NaN — the lowest unmasked index —
    # wins each step with a NaN gain, and the steps go on: the other draws' incumbents still move
    omega, phase, w, eps = c.groups[0]
    wn = w.copy()
    wn[2, 5] = np.nan
    out = c.run(engine, 4, groups=[(omega, phase, wn, eps), c.groups[1]])
    assert np.isnan(out[3][2]).all() and np.isnan(out[2][2]) and np.isfinite(np.delete(out[3], 2, axis=0)).all()
    assert out[0].tolist() == [0, 1, 2, 3] and np.isnan(out[1]).all()
    replay(c, out, 4, "a NaN weight")
    # a NaN candidate: its key is NaN, it wins step 0, is masked (+inf) from step 1 on, and the later steps are the greedy's
    k = next(i for i in range(c.M - 1, -1, -1) if i not in base[0][:3])      # (not one of the picks the later steps are compared with)
    Xn = c.Xc.copy()
    Xn[k, 1] = np.nan
    engine.set_candidates(Xn)
    out = c.run(engine, 4)
    assert out[0][0] == k and np.isnan(out[1][0]) and np.isfinite(out[1][1:]).all() and out[4][1][k] == np.inf
    assert np.array_equal(out[2], base[2])                          # a NaN value leaves every incumbent as it was
    assert np.array_equal(out[0][1:], base[0][:3]) and np.array_equal(out[1][1:], base[1][:3])
    replay(c, out, 4, "a NaN candidate")
    # every candidate twice: the copies' values are the originals' bits, ties go to the lowest index
    engine.set_candidates(np.vstack([c.Xc, c.Xc]))
    two = c.run(engine, 6)
    assert np.array_equal(two[3][:, :c.M], base[3]) and np.array_equal(two[3][:, c.M:], base[3])
    assert two[0][0] == base[0][0] and two[1][0] == base[1][0] and np.array_equal(two[4][0][:c.M], base[4][0])
    replay(c, two, 6, "every candidate twice")


# ---- a reader --------------------------------------------------------------------------------------------------------------------------
def test_reader_only(engine):
    eng = engine
    c = case_of("n130-m257-f65-d5-3x16-p64")
    plain = Case(130, 257, 65, 5, 3, 16, 64, F.MATERN15, True, "fp64", "plain", 0)      # (an unscaled slot: fit_append below)

    def fit():
        eng.fit(plain.X, plain.yn, plain.kind, plain.ls, NOISE)
        eng.set_candidates(plain.Xc)

    fit()
    eng.posterior(0, Y_MEAN, Y_STD, fetch=False)
    eng.take_negative_variance_flag()
    before = eng.acq_argbest(O.UCB, 2.576, k_seeds=8, return_values=True)
    plain.run(eng, 8)
    after = eng.acq_argbest(O.UCB, 2.576, k_seeds=8, return_values=True)      # still answers, from the posterior before the call
    assert before[0] == after[0] and before[1] == after[1] and np.array_equal(before[2], after[2])
    assert np.array_equal(before[3], after[3]) and np.array_equal(before[4], after[4])
    assert np.array_equal(eng.get_candidate_rows(np.arange(c.M), c.d), plain.Xc)
    assert eng.take_negative_variance_flag() is False
    # an append, the greedy over the grown model, and the refresh still takes its incremental route, to the bits it gives without
    x_new = np.random.RandomState(5).uniform(size=(2, c.d))
    yn2 = np.concatenate([plain.yn, [0.2, -0.4]])
    groups2 = [(om, ph, w, np.hstack([eps, np.zeros((plain.S, 2))])) for om, ph, w, eps in plain.groups]

    def arm():
        fit()
        eng.posterior(0, Y_MEAN, Y_STD, fetch=False)
        eng.fit_append(x_new, yn2)

    arm()
    mu_a, sd_a, route_a = eng.posterior_refresh(0, Y_MEAN, Y_STD, return_route=True)
    arm()
    plain.run(eng, 8, groups=groups2)
    mu_b, sd_b, route_b = eng.posterior_refresh(0, Y_MEAN, Y_STD, return_route=True)
    assert route_a == 1 and route_b == 1
    assert np.array_equal(mu_a, mu_b) and np.array_equal(sd_a, sd_b)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(engine):
    eng = engine
    c = case_of("n65-m63-f64-d2-2x5-p1")
    c.fit(eng)
    G, S, Fn, N, d = c.G, c.S, c.F, c.N, c.d
    omega = np.ascontiguousarray(np.concatenate([g[0].ravel() for g in c.groups]))
    phase = np.ascontiguousarray(np.concatenate([g[1] for g in c.groups]))
    w = np.ascontiguousarray(np.concatenate([g[2].ravel() for g in c.groups]))
    eps = np.ascontiguousarray(np.concatenate([g[3].ravel() for g in c.groups]))
    pend = np.ascontiguousarray(c.pending)
    pi, pg, bl = np.empty(64, dtype=np.int64), np.empty(64), np.empty(256)

    def call(h=None, slot=0, y_mean=Y_MEAN, y_std=Y_STD, n_groups=G, n_paths=S, n_features=Fn, draws=None, noisy=1, y_best=0.0,
             pending=dptr(pend), n_pending=1, dd=d, q=4, outs=None):
        draws = [dptr(omega), dptr(phase), dptr(w), dptr(eps)] if draws is None else draws
        outs = [iptr(pi), dptr(pg), dptr(bl)] if outs is None else outs
        return eng._lib.gpbo_qnei_greedy(eng._h if h is None else h, slot, y_mean, y_std, n_groups, n_paths, n_features, *draws, noisy,
                                         y_best, pending, n_pending, dd, q, 0, *outs, None, None)

    assert call() == _lib.GPBO_OK
    # n_groups outside [1, GPBO_MAX_QNEI_GROUPS]
    assert call(n_groups=0) == _lib.ERR_INVALID and call(n_groups=17) == _lib.ERR_INVALID
    # n_paths or n_features outside gpbo_sample_paths' ranges
    assert call(n_paths=0) == _lib.ERR_INVALID and call(n_paths=17) == _lib.ERR_INVALID
    assert call(n_features=0) == _lib.ERR_INVALID and call(n_features=4097) == _lib.ERR_INVALID
    # a NULL among the draw inputs, pick_idx, pick_gain or baseline_out
    for k in range(4):
        a = [dptr(omega), dptr(phase), dptr(w), dptr(eps)]
        a[k] = None
        assert call(draws=a) == _lib.ERR_INVALID
    for k in range(3):
        a = [iptr(pi), dptr(pg), dptr(bl)]
        a[k] = None
        assert call(outs=a) == _lib.ERR_INVALID
    # y_std not finite or not positive, y_mean not finite
    for bad in (0.0, -1.0, np.inf, np.nan):
        assert call(y_std=bad) == _lib.ERR_INVALID
    for bad in (np.inf, np.nan):
        assert call(y_mean=bad) == _lib.ERR_INVALID
    # noisy == 0 with a non-finite y_best (and noisy != 0 does not read it)
    for bad in (np.inf, -np.inf, np.nan):
        assert call(noisy=0, y_best=bad) == _lib.ERR_INVALID
        assert call(noisy=1, y_best=bad) == _lib.GPBO_OK
    # n_pending outside [0, GPBO_MAX_QNEI_POINTS], n_pending > 0 with NULL or non-finite pending, d not the slot's
    assert call(n_pending=-1) == _lib.ERR_INVALID and call(n_pending=65) == _lib.ERR_INVALID
    assert call(pending=None, n_pending=1) == _lib.ERR_INVALID
    assert call(pending=None, n_pending=0) == _lib.GPBO_OK
    for bad in (np.nan, np.inf):
        pb = pend.copy()
        pb[0, 1] = bad
        assert call(pending=dptr(pb)) == _lib.ERR_INVALID
    assert call(dd=d + 1) == _lib.ERR_INVALID and call(dd=d + 1, pending=None, n_pending=0) == _lib.ERR_INVALID
    # q outside [1, GPBO_MAX_SEEDS], or q > M
    assert call(q=0) == _lib.ERR_INVALID and call(q=65) == _lib.ERR_INVALID
    assert call(q=63) == _lib.GPBO_OK and call(q=64) == _lib.ERR_INVALID             # M = 63
    # the engine's own refusals, as exceptions
    with pytest.raises(ValueError, match="n_groups"):
        eng.qnei_greedy(c.groups * 9, 2)
    with pytest.raises(ValueError, match="same S and F"):
        eng.qnei_greedy([c.groups[0], (c.groups[1][0], c.groups[1][1], c.groups[1][2][:2], c.groups[1][3][:2])], 2)
    with pytest.raises(ValueError, match="pending"):
        eng.qnei_greedy(c.groups, 2, pending=np.zeros((1, d + 1)))
    with pytest.raises(ValueError, match="q out of range"):
        eng.qnei_greedy(c.groups, 65)
    # GPBO_ERR_STATE: a slot that gpbo_lml left unfitted
    eng.fit(c.X, c.yn, c.kind, c.ls, NOISE, slot=3)
    eng.lml(c.X, c.yn, c.kind, c.ls, NOISE, slot=3)
    with pytest.raises(GpboError, match="not been fitted"):
        eng.qnei_greedy(c.groups, 2, slot=3)
    assert call(slot=3) == _lib.ERR_STATE
    # ... a fit pending on the slot (the engine would wait for it: asked at the C boundary)
    with eng.overlapped_fits():
        eng.fit(c.X, c.yn, c.kind, c.ls, NOISE)
        assert call() == _lib.ERR_STATE
    # ... candidates of another d
    eng.set_candidates(np.random.RandomState(1).uniform(size=(10, d + 1)))
    with pytest.raises(GpboError, match="dimension"):
        eng.qnei_greedy(c.groups, 2, y_mean=Y_MEAN, y_std=Y_STD)
    # ... no resident candidates: a context that never had any
    fresh = GpEngine(0)
    try:
        assert call(h=fresh._h, slot=5) == _lib.ERR_STATE
        fresh.fit(c.X, c.yn, c.kind, c.ls, NOISE)
        with pytest.raises(GpboError, match="no candidates"):
            fresh.qnei_greedy(c.groups, 2, y_mean=Y_MEAN, y_std=Y_STD)
    finally:
        fresh.close()
    # a device group
    with pytest.raises(NotImplementedError, match="device group"):
        GroupEngine.qnei_greedy(object.__new__(GroupEngine), c.groups, 2)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_suggest_qnei_picks_the_replays_picks(engine, monkeypatch):
    D, N, M, q, n_draws, FEATURES = 3, 30, 257, 4, 20, 128
    bounds = np.array([[0.0, 1.0]] * D)
    X = np.random.RandomState(130).uniform(size=(N, D))
    y = np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1]) + X[:, 2] ** 2 + 0.05 * np.random.RandomState(131).standard_normal(N)
    drv = B.Driver(engine, X, y, bounds, A.UpperConfidenceBound(kappa=2.576), seed=7, n_random=M)
    seen = {}
    real = engine.qnei_greedy

    def recording(groups, q_, **kw):
        kw.update(return_values=True, return_keys=True)
        seen["groups"], seen["kw"] = groups, kw
        seen["out"] = real(groups, q_, **kw)
        return seen["out"]

    monkeypatch.setattr(engine, "qnei_greedy", recording)
    pending = [{"x0": 0.25, "x1": 0.5, "x2": 0.75}]
    picks, info = suggest_qnei(drv, q, n_random=M, n_draws=n_draws, n_features=FEATURES, pending=pending, return_info=True)
    G, S = draw_layout(n_draws)
    idx, gain, m0, values, keys = seen["out"]
    assert (G, S) == (2, 10) and values.shape == (20, M) and info["n_draws"] == 20 and len(seen["groups"]) == 2
    assert np.array_equal(seen["kw"]["pending"], [[0.25, 0.5, 0.75]]) and seen["kw"]["noisy"] is True
    t_idx, t_gain, t_keys, _ = Q.greedy(values, m0, q)
    assert np.array_equal(keys, t_keys, equal_nan=True)
    assert np.array_equal(info["index"], t_idx) and np.array_equal(info["gain"], t_gain) and np.array_equal(info["baseline"], m0)
    Xc = engine.get_candidate_rows(np.arange(M), D)                           # the one candidate draw is still resident
    assert np.array_equal(np.array([list(p.values()) for p in picks]), Xc[t_idx])
    assert B.rows_to_indices(picks, Xc).tolist() == t_idx.tolist() and info["gain"][0] > 0.0
    # the documented draws, replayed on a twin RandomState (the values against the truth's for them: printed; parity is held to its
    # bar in test_parity_and_exact_replay)
    twin = B.Driver(engine, X, y, bounds, A.UpperConfidenceBound(kappa=2.576), seed=7, n_random=M)
    twin._gp.fit(twin._space.params, twin._space.target)
    rng, gp = twin._random_state, drv._gp
    assert np.array_equal(np.column_stack([rng.uniform(0.0, 1.0, M) for _ in range(D)]), Xc)
    groups = []
    for _ in range(G):
        omega, phase = spectral_draw(gp._kind, FEATURES, D, rng)
        w = rng.standard_normal((S, FEATURES))
        groups.append((omega, phase, w, rng.standard_normal((S, N)) * np.sqrt(float(gp.alpha))))
    assert B.same_state(drv._random_state, rng)
    yn = (y - gp._y_train_mean) / gp._y_train_std
    pts = np.vstack([Xc, X, [[0.25, 0.5, 0.75]]])
    ref = Q.group_values(P.paths_cho, int(gp._kind), X, yn, np.array(gp._ls), float(gp.alpha), groups, pts, gp._y_train_mean,
                         gp._y_train_std)
    scale = float(gp._y_train_std) * max(1.0, float(np.abs((ref - gp._y_train_mean) / gp._y_train_std).max()))
    print(f"values {np.abs(values - ref[:, :M]).max() / scale:.2e}, baselines "
          f"{np.abs(m0 - Q.baseline(ref[:, M:M + N], ref[:, M + N:])).max() / scale:.2e} of the scale")
    # gp.predict answers for the real data afterwards
    Xq = np.random.RandomState(9).uniform(size=(20, D))
    mu1, sd1 = drv._gp.predict(Xq, return_std=True)
    mu0, sd0 = twin._gp.predict(Xq, return_std=True)
    assert np.array_equal(mu0, mu1) and np.array_equal(sd0, sd1) and drv._gp.X_train_.shape[0] == N
