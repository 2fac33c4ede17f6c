"""GPU (-m gpu): gpmo3_nhvi_greedy against tests/qnehvi3_truth.py and `multiobjective.hypervolume`: the decomposition on raw values
(fronts and cells exactly; the cell sum within 8 (2 n + 3) eps hypervolume(front u y): both sides are sums of at most 2 n + 3
non-negative terms of a few roundings each), the exact replay of the greedy on the device's own values, fronts and cells, the leading
picks against the independent truth (tests/paths_truth.py) where the truth itself separates them, and the reader contract."""
import functools

import numpy as np
import pytest

import batch_truth as B
import matern_family_truth as F
import paths_truth as P
import qnehvi3_truth as Q3
import qnehvi_truth as Q
from bayesianoptimization_amd.engine import F32
from bayesianoptimization_amd.multiobjective import hypervolume
from bayesianoptimization_amd.thompson import spectral_draw
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
REF = np.array([-0.5, 0.25, 0.0])
NAN = np.nan


# ---- the decomposition on raw values -------------------------------------------------------------------------------------------------
def _anti(n):
    """n triples that no other dominates: an antichain in objectives (0, 1), objective 2 varied"""
    k = np.arange(1.0, n + 1)
    return np.column_stack([k, n + 1 - k, 1.0 + k % 5])


def _grid(T, n, seed):
    return np.round((REF + np.random.RandomState(seed).uniform(-0.2, 2.0, (T, n, 3))) * 4) / 4


#: name -> (base (T, n, 3), inserts (T, n_insert, 3) or None, ref, the front sizes the case is meant to have: (min, max) over the draws)
ZERO = np.zeros(3)
DECOMP = {
    "empty": (REF + np.array([[[0.0, 1.0, 1.0], [1.0, -1.0, 1.0], [1.0, 1.0, 0.0], [NAN, 1.0, 1.0]]]), None, REF, (0, 0)),
    "one-point": (REF + np.array([[[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [0.5, 2.0, 3.0]]]), None, REF, (1, 1)),
    "ties-on-a-grid-256-draws": (_grid(256, 40, 0), None, REF, (1, 40)),
    "dominated-only-in-3d": (np.array([[[2.0, 2.0, 1.0], [1.0, 1.0, 2.0], [1.0, 1.0, 0.5], [2.0, 1.0, 1.0]]]), None, ZERO, (2, 2)),
    "insert-removes-several": (_anti(6)[None], np.array([[[4.5, 5.5, 7.0]]]), ZERO, (4, 4)),      # (2, 5, .), (3, 4, .), (4, 3, .) leave
    "insert-changes-nothing": (_anti(6)[None], np.array([[[1.0, 6.0, 2.0], [0.5, 0.5, 0.5], [NAN, 9.0, 9.0], [9.0, 9.0, 0.0]]]), ZERO, (6, 6)),
    "inserts-on-a-grid": (_grid(7, 30, 1), _grid(7, 9, 2), REF, (3, 39)),
    "full-128": (np.vstack([_anti(128)[::-1], [[0.5, 0.5, 0.5]]])[None], None, ZERO, (128, 128)),
    "full-128-insert-dominates-three": (_anti(128)[None], np.array([[[5.5, 126.5, 9.0]]]), ZERO, (126, 126)),
}


@pytest.mark.parametrize("name", list(DECOMP))
def test_decomposition_against_hypervolume(debug_engine, name):
    base, ins, ref, (lo, hi) = DECOMP[name]
    T = base.shape[0]
    want = [Q3.front_of(base[t], ref) for t in range(T)]
    for i in range(0 if ins is None else ins.shape[1]):
        want = [Q3.insert(f, ins[t, i], ref)[0] for t, f in enumerate(want)]
    sizes = [f.shape[0] for f in want]
    assert lo <= min(sizes) and max(sizes) <= hi and len(set(sizes)) >= min(T, 2), sizes      # on the reference alone
    size, fronts, count, cells = debug_engine.debug_qnehvi3_cells(np.ascontiguousarray(base.transpose(2, 0, 1)), ref,
                                                                 None if ins is None else np.ascontiguousarray(ins.transpose(2, 0, 1)))
    got, got_cells = Q.unpack(size, fronts), Q.unpack(count, cells)
    assert Q3.same_rows(got, want), f"{name}: fronts differ (sizes {size.tolist()[:8]}, want {sizes[:8]})"
    assert all(c.shape[0] <= 2 * f.shape[0] + 1 for c, f in zip(got_cells, got))
    assert Q3.same_rows(got_cells, [Q3.sweep(f, ref) for f in want]), f"{name}: the cells are not the sweep's"
    rs = np.random.RandomState(5)
    worst = 0.0
    for t in range(0, T, 16):
        f = want[t]
        probes = np.vstack([ref + rs.uniform(-0.2, 2.2, (4, 3)), np.round((ref + rs.uniform(-0.2, 2.2, (4, 3))) * 4) / 4, f[:2],
                            f.max(axis=0, initial=1.0)[None] + 1.0])
        hv0 = hypervolume(f, ref) if f.shape[0] else 0.0
        sums = Q3.hvi(probes.T, got_cells[t])
        for y, s in zip(probes, sums):
            hv1 = hypervolume(np.vstack([f, y[None]]), ref)
            bar = 8 * (2 * f.shape[0] + 3) * EPS * hv1
            worst = max(worst, abs(s - (hv1 - hv0)) / bar if bar else float(s != hv1 - hv0))
            assert abs(s - (hv1 - hv0)) <= bar, f"{name}: draw {t}, y {y.tolist()}: {s!r} against {hv1 - hv0!r}, bar {bar:.1e}"
    print(f"{name}: fronts of {min(sizes)}..{max(sizes)} points, worst error {worst:.2g} of its bar")


def test_one_point_above_the_cap_is_refused(debug_engine):
    run = lambda base, ins=None: debug_engine.debug_qnehvi3_cells(np.ascontiguousarray(base.transpose(2, 0, 1)), np.zeros(3), ins)
    with pytest.raises(NotImplementedError, match="draw 1 outgrew 128"):
        run(np.stack([np.vstack([_anti(128), [[0.5, 0.5, 0.5]]]), _anti(129)]))
    with pytest.raises(NotImplementedError, match="draw 0 outgrew 128"):
        run(_anti(128)[None], np.array([[[0.5]], [[200.0]], [[1.0]]]))
    assert run(_anti(128)[None])[0].tolist() == [128]      # ... and a call after a refusal works


# ---- the whole call ----------------------------------------------------------------------------------------------------------------
NOISE = 1e-2
Y_MEAN, Y_STD = (3.5, -1.0, 0.25), (0.4, 2.0, 1.5)

#: name -> (M, F, d, G, S, pending points or None for no base at all, seed, three slots (N, kind, variant))
CASES = {
    "m1-1x1-b0": (1, 1, 1, 1, 1, None, 0, ((1, F.RBF, "plain"),) * 3),
    "m63-2x5-p1": (63, 64, 2, 2, 5, 1, 0, ((65, F.MATERN25, "plain"),) * 3),                        # odd M, T under one LDS stage
    "m64-16x16-p0": (64, 33, 3, 16, 16, 0, 0, ((64, F.RBF, "plain"), (64, F.MATERN25, "plain"), (40, F.MATERN15, "plain"))),
    "m1030-3x16-p40": (1030, 65, 5, 3, 16, 40, 0, ((130, F.MATERN15, "plain"), (65, F.RBF, "f32"), (97, F.MATERN25, "plain"))),
}
PICK_CASES = ["m63-2x5-p1", "m1030-3x16-p40"]


class Case:
    """Data, draws and the independent truth of one case (computed once, shared, never changed)."""

    def __init__(self, M, Fn, d, G, S, pending, seed, slots):
        self.M, self.d, self.G, self.S, self.T = M, d, G, S, G * S
        N0 = max(s[0] for s in slots)
        X, y0 = F.data(N0, d, seed=seed + 17 * N0 + d)
        ys = [y0, np.cos(3.0 * X.sum(1) + 0.7), np.sin(2.0 * X[:, 0]) - 0.5 * X.sum(1)]
        rs = np.random.RandomState(3000 + seed + N0 + M + Fn)
        self.Xc = rs.uniform(size=(M, d))
        self.base = None if pending is None else np.vstack([X, rs.uniform(size=(pending, d))])
        self.slots = []
        for j, (n, kind, variant) in enumerate(slots):
            yn = (ys[j][:n] - ys[j][:n].mean()) / ys[j][:n].std() if n > 1 else np.array([0.3 - 0.5 * j])
            ls = (0.5, 0.7, 0.6)[j] * np.sqrt(d) * (np.geomspace(0.75, 1.33, d) if d > 1 else np.ones(1))
            groups = []
            for _ in range(G):
                omega, phase = spectral_draw(kind, Fn, d, rs)
                groups.append((omega, phase, rs.standard_normal((S, Fn)), rs.standard_normal((S, n)) * np.sqrt(NOISE)))
            self.slots.append((X[:n], yn, kind, ls, variant, groups))
        self.draws = [s[5] for s in self.slots]
        self.refp = np.array([Y_MEAN[j] + Y_STD[j] * float(np.quantile(s[1], 0.25)) for j, s in enumerate(self.slots)])

    def truth(self, pts):
        """(3, T, len(pts)) by paths_truth's Cholesky route"""
        return np.stack([Q.group_values(P.paths_cho, kind, X, yn, ls, NOISE, groups, pts, Y_MEAN[j], Y_STD[j])
                         for j, (X, yn, kind, ls, _, groups) in enumerate(self.slots)])

    def fit(self, eng):
        for j, (X, yn, kind, ls, variant, _) in enumerate(self.slots):
            eng.fit(X, yn, kind, ls, NOISE, slot=j, precision=F32 if variant == "f32" else 0)
        eng.set_candidates(self.Xc)

    def run(self, eng, q, **kw):
        kw.setdefault("base", self.base)
        return eng.qnehvi3_greedy(self.draws, q, self.refp, y_mean=Y_MEAN, y_std=Y_STD, return_values=True, return_keys=True,
                                  return_fronts=True, **kw)


@functools.lru_cache(maxsize=None)
def case_of(name):
    return Case(*CASES[name])


def replay(c, out, q, what):
    """fronts_out[0] is the front of base_values_out and cells_out[0] its sweep; then the restated greedy on the device's own values,
    fronts and cells: keys bit for bit, picks, gains, fronts_out[1] and cells_out[1] exactly"""
    T = out["values"].shape[1]
    f0, f1 = (Q.unpack(out["front_size"][k], out["fronts"][k]) for k in range(2))
    c0, c1 = (Q.unpack(out["cell_count"][k], out["cells"][k]) for k in range(2))
    built = Q3.fronts_of(out["base_values"], c.refp) if out["base_values"].shape[2] else [np.empty((0, 3))] * T
    assert Q3.same_rows(f0, built), f"{what}: fronts_out[0] is not the front of base_values_out"
    assert Q3.same_rows(c0, [Q3.sweep(f, c.refp) for f in f0]), f"{what}: cells_out[0] is not the sweep of fronts_out[0]"
    t_idx, t_gain, t_keys, t_f, t_c = Q3.greedy(out["values"], f0, c0, c.refp, q)
    keys = out["keys"]
    assert np.array_equal(keys, t_keys, equal_nan=True), f"{what}: keys differ at {np.argwhere(~((keys == t_keys) | (np.isnan(keys) & np.isnan(t_keys))))[:4].tolist()}"
    assert np.array_equal(out["index"], t_idx), f"{what}: picks {out['index'].tolist()}, replay {t_idx.tolist()}"
    assert np.array_equal(out["gain"], t_gain, equal_nan=True) and not np.signbit(out["gain"][out["gain"] == 0.0]).any()
    assert Q3.same_rows(f1, t_f) and Q3.same_rows(c1, t_c), f"{what}: the fronts or cells after the last pick are not the replay's"
    return out["cell_count"]


@pytest.mark.parametrize("name", list(CASES))
def test_exact_replay(engine, name):
    c = case_of(name)
    c.fit(engine)
    q = min(8, c.M)
    out = c.run(engine, q)
    counts = replay(c, out, q, name)
    print(f"{name}: {counts[0].min()}..{counts[0].max()} cells a draw before, {counts[1].min()}..{counts[1].max()} after; "
          f"{counts[1].sum()} in all")
    if name == "m64-16x16-p0":      # several LDS stages of 1008 cells, and a boundary between draws of different sizes
        assert counts[0].sum() > 2 * 1008 and len(set(counts[0].tolist())) > 4


def test_replay_no_base_nan_candidate_q_equals_m_and_the_plain_draws(engine):
    c = case_of("m63-2x5-p1")
    c.fit(engine)
    base = c.run(engine, 4)
    none = c.run(engine, 4, base=None)
    assert (none["front_size"][0] == 0).all() and (none["cell_count"][0] == 1).all() and np.array_equal(none["values"], base["values"])
    replay(c, none, 4, "no base")
    for j, (_, _, _, _, _, groups) in enumerate(c.slots):      # rows [g S, (g + 1) S) are gpbo_sample_paths' bits for slot j, group g
        for g, (omega, phase, w, eps) in enumerate(groups):
            _, _, plain = engine.sample_paths(omega, phase, w, eps, slot=j, y_mean=Y_MEAN[j], y_std=Y_STD[j], return_values=True)
            assert np.array_equal(base["values"][j, g * c.S:(g + 1) * c.S], plain), f"objective {j} group {g}"
    k = next(i for i in range(c.M - 1, -1, -1) if i not in base["index"][:3])
    Xn = c.Xc.copy()
    Xn[k, 1] = np.nan
    engine.set_candidates(Xn)
    out = c.run(engine, 4)
    assert out["index"][0] == k and np.isnan(out["gain"][0]) and out["keys"][1][k] == np.inf
    assert np.array_equal(out["index"][1:], base["index"][:3]) and np.array_equal(out["gain"][1:], base["gain"][:3])
    replay(c, out, 4, "a NaN candidate")
    engine.set_candidates(c.Xc[:5])
    out = c.run(engine, 5)
    replay(c, out, 5, "q = M = 5")
    assert sorted(out["index"].tolist()) == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("name", PICK_CASES)
def test_leading_picks_against_the_truth(engine, name):
    c = case_of(name)
    q = 6
    f0 = Q3.fronts_of(c.truth(c.base), c.refp)
    t_idx, _, t_keys, _, _ = Q3.greedy(c.truth(c.Xc), f0, [Q3.sweep(f, c.refp) for f in f0], c.refp, q)
    n, gaps = Q.leading_separated_steps(t_keys, B.GAP_FLOOR)
    print(f"{name}: truth picks {t_idx.tolist()}, gaps {['%.1e' % g for g in gaps]}: {n} leading separated steps")
    assert n >= 2, f"{name}: only {n} separated leading steps in the truth itself: pick another seed"
    c.fit(engine)
    out = c.run(engine, q)
    assert np.array_equal(out["index"][:n], t_idx[:n]), f"{name}: picks {out['index'][:n].tolist()}, truth {t_idx[:n].tolist()}"


def test_reader_only(engine):
    eng, c = engine, case_of("m63-2x5-p1")
    c.fit(eng)
    alpha = [eng.get_alpha(c.slots[j][0].shape[0], slot=j) for j in range(3)]
    post = [eng.posterior(j, Y_MEAN[j], Y_STD[j]) for j in range(3)]
    eng.take_negative_variance_flag()
    before = eng.acq_argbest(O.UCB, 2.576, k_seeds=8, return_values=True)
    c.run(eng, 8)
    after = eng.acq_argbest(O.UCB, 2.576, k_seeds=8, return_values=True)      # still answers, from the posterior before the call
    assert before[0] == after[0] and before[1] == after[1] and all(np.array_equal(a, b) for a, b in zip(before[2:], after[2:]))
    assert all(np.array_equal(eng.get_alpha(c.slots[j][0].shape[0], slot=j), alpha[j]) for j in range(3))
    assert np.array_equal(eng.get_candidate_rows(np.arange(c.M), c.d), c.Xc)
    assert eng.take_negative_variance_flag() is False
    for j in range(3):
        mu, sd = eng.posterior(j, Y_MEAN[j], Y_STD[j])
        assert np.array_equal(mu, post[j][0]) and np.array_equal(sd, post[j][1])
