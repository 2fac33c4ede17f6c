"""CPU: expected hypervolume improvement's host side — `box_decomposition` against a brute-force hypervolume improvement that shares
no code with it, the fp64 restatement (tests/ehvi_truth.py: `ehvi_values`) against the 60-digit mpmath truth and against Monte Carlo,
`hypervolume` / `pareto_front` against brute force, and `ParetoOptimizer` over an oracle-backed engine double: the call order, the
RandomState it leaves behind, the refusals and their order.  The device's arithmetic is checked in tests/test_gpu_ehvi.py."""
import os
import re

import numpy as np
import pytest

import batch_truth as B
import ehvi_truth as T
from bayesianoptimization_amd import _lib
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd.multiobjective import MAX_FRONT, ParetoOptimizer, box_decomposition, hypervolume, pareto_front
from conftest import ROOT
from helpers import FakeEngine


def _points_around(front, ref, m, n, seed):
    """n points at which the improvement is asked: around the front, on its points, on and below the reference point"""
    rs = np.random.RandomState(seed)
    pts = rs.uniform(ref - 0.2, 1.3, size=(n, m))
    if front.shape[0]:
        pts[0] = front[0]                                   # on a front point: no improvement
        pts[1] = front[-1] + 0.05                           # dominating one
        pts[2, 0] = front[front.shape[0] // 2, 0]           # a coordinate on a level
    pts[3] = ref                                            # on the reference point
    pts[4] = ref - 0.1                                      # below it
    pts[5] = np.r_[ref[0], np.full(m - 1, 1.2)]             # on its boundary in one objective
    return pts


def _decomposition_case(front, ref, seed, n=24):
    m = ref.shape[0]
    n_levels, levels, lo, hi = box_decomposition(front, ref)
    rows = T.trim(n_levels, levels)
    # the shape of the result
    assert levels.shape == (m, _lib.MAX_EHVI_LEVELS) and lo.shape == hi.shape and lo.shape[1] == m
    assert lo.shape[0] == int(np.prod(n_levels[:-1] - 1))
    assert (lo < hi).all() and (lo >= 0).all() and (hi < n_levels[None, :]).all()
    for j, r in enumerate(rows):
        assert r[0] == ref[j] and np.isposinf(r[-1]) and np.isfinite(r[:-1]).all() and (np.diff(r) > 0).all()
        assert np.array_equal(r[1:-1], np.unique(front[:, j])) and np.isposinf(levels[j, n_levels[j]:]).all()
    assert (hi[:, :m - 1] == lo[:, :m - 1] + 1).all() and (hi[:, m - 1] == n_levels[m - 1] - 1).all()
    # disjoint: the boxes differ in their cell of the grid over objectives 0 .. m - 2
    assert np.unique(lo[:, :m - 1], axis=0).shape[0] == lo.shape[0]
    # the improvement of a point: the cell sum with every sd zero, against the brute force
    pts = _points_around(front, ref, m, n, seed)
    got = T.ehvi_values(pts.T, np.zeros((m, n)), rows, lo, hi)
    want = np.array([T.hvi_brute(front, ref, y) for y in pts])
    assert want[:2].max() == 0.0 or front.shape[0] == 0 or want[1] > 0.0
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, want.max()), (front.shape, np.abs(got - want).max())
    assert (want > 0).sum() >= n // 3
    return lo.shape[0]


@pytest.mark.parametrize("m", [2, 3])
def test_box_decomposition_against_brute_force(m):
    ref = np.full(m, 0.1) + 0.05 * np.arange(m)
    cells = [_decomposition_case(T.random_front(n, m, seed=10 * m + n, lo=0.3), ref, seed=n, n=24 if n < 100 else 10)
             for n in (0, 1, 11, 128)]
    assert cells == ([1, 2, 12, 129] if m == 2 else [1, 4, 144, 129 * 129])
    # duplicated values in one objective (m = 3: only there can non-dominated points share one)
    if m == 3:
        front = pareto_front(np.array([[0.9, 0.4, 0.5], [0.9, 0.5, 0.4], [0.4, 0.9, 0.5], [0.5, 0.9, 0.4], [0.6, 0.6, 0.8],
                                       [0.6, 0.7, 0.7]]), ref)
        assert front.shape[0] == 6
        n_levels, _, lo, _ = box_decomposition(front, ref)
        assert n_levels.tolist() == [6, 7, 6] and lo.shape[0] == 30
        _decomposition_case(front, ref, seed=4)
    # a front that is not above the reference point, or not finite, is refused
    with pytest.raises(ValueError, match="strictly above"):
        box_decomposition(np.r_[ref[:-1] + 0.1, ref[-1]][None], ref)
    with pytest.raises(ValueError, match="finite"):
        box_decomposition(np.full((1, m), np.inf), ref)
    with pytest.raises(ValueError, match="2 or 3"):
        box_decomposition(np.ones((1, 4)), np.zeros(4))
    with pytest.raises(ValueError, match="distinct front values"):
        box_decomposition(T.random_front(129, m, seed=1), ref)


@pytest.mark.parametrize("m, n", [(2, 11), (3, 20)])
def test_restatement_against_the_mpmath_truth_and_monte_carlo(m, n):
    ref = np.zeros(m)
    front = T.random_front(n, m, seed=n)
    n_levels, levels, lo, hi = box_decomposition(front, ref)
    rows = T.trim(n_levels, levels)
    assert lo.shape[0] == (12 if m == 2 else 441)
    rs = np.random.RandomState(m)
    M = 12
    mu = rs.uniform(-0.2, 1.1, size=(m, M))
    sd = rs.uniform(0.02, 0.4, size=(m, M))
    mu[:, 0], sd[:, 0] = -0.6, 0.1                           # far below the front: every z in the tail form (-8 and below)
    mu[0, 1], sd[0, 1] = 0.9, 0.0                            # one clipped objective
    got, scale = T.ehvi_values(mu, sd, rows, lo, hi, return_scale=True)
    truth = np.array([T.ehvi_truth(mu[:, i], sd[:, i], rows, lo, hi) for i in range(M)])
    worst, ok = T.within_bar(got, truth[:, 0], truth[:, 1])
    rel = np.abs(got - truth[:, 0]) / np.maximum(truth[:, 0], T.TINY)
    print(f"m={m}: worst error / bar {worst:.2e}; worst relative error {rel.max():.2e}; S / EHVI {scale[2:] / got[2:]}")
    assert ok and (got >= 0).all() and np.abs(scale - truth[:, 1]).max() <= 1e-12 * truth[:, 1].max()
    assert 0.0 < truth[0, 0] < 1e-20 and rel[0] <= 1e-9     # the tail keeps its relative accuracy
    # Monte Carlo: the mean improvement of 1e5 draws (the cell sum with sd = 0, held to the brute force above)
    S = 100_000
    for i in np.argsort(-got[2:])[:3] + 2:                   # the three largest: an improvement the draws do hit
        draws = mu[:, i, None] + sd[:, i, None] * rs.standard_normal((m, S))
        hvi = T.ehvi_values(draws, np.zeros((m, S)), rows, lo, hi)
        se = hvi.std(ddof=1) / np.sqrt(S)
        print(f"m={m} candidate {i}: EHVI {got[i]:.6e}, Monte Carlo {hvi.mean():.6e} +- {se:.1e}")
        assert se > 0.0 and abs(hvi.mean() - got[i]) <= 4.0 * se


def test_conventions_of_the_restatement():
    ref = np.zeros(2)
    front = T.random_front(5, 2, seed=5)
    n_levels, levels, lo, hi = box_decomposition(front, ref)
    rows = T.trim(n_levels, levels)
    mu = np.array([[0.5, np.nan, 0.5, 0.5], [0.5, 0.5, 0.5, 1.5]])
    sd = np.array([[0.1, 0.1, np.nan, 0.0], [0.1, 0.1, 0.1, 0.0]])
    v = T.ehvi_values(mu, sd, rows, lo, hi)
    assert v[0] > 0 and np.isnan(v[1]) and np.isnan(v[2])
    assert v[3] == pytest.approx(T.hvi_brute(front, ref, mu[:, 3]), rel=1e-13)
    assert T.f_values(np.array([-40.0, -np.inf]))[0] == 0.0 and T.f_values(np.array([-np.inf]))[0] == 0.0
    for z in (-38.0, -28.5, -27.5, -5.0, -1.001, -0.999, 0.0, 6.0):
        assert abs(T.f_values(np.array([z]))[0] - float(T.f_truth(z))) <= 1e-13 * float(T.f_truth(z))


@pytest.mark.parametrize("m", [2, 3])
def test_hypervolume_and_pareto_front_against_brute_force(m):
    rs = np.random.RandomState(m)
    ref = np.full(m, 0.25)
    for n in (0, 1, 2, 7, 40):
        Y = np.round(rs.uniform(0.0, 1.0, size=(n, m)), 1 if n == 40 else 3)      # n = 40: ties and duplicates
        if n >= 7:
            Y[3] = Y[1]                                      # a duplicate row
            Y[4] = ref                                       # on the reference point
            Y[5, 0] = ref[0]                                 # on its boundary
        P = pareto_front(Y, ref)
        assert np.array_equal(P, T.front_brute(Y, ref))
        hv = hypervolume(Y, ref)
        assert abs(hv - T.hv_brute(Y, ref)) <= 1e-13 and abs(hv - hypervolume(P, ref)) <= 1e-15
    assert hypervolume(np.array([[1.0, 2.0, 3.0][:m]]), np.zeros(m)) == [2.0, 6.0][m - 2]
    with pytest.raises(ValueError):
        hypervolume(np.ones((1, 4)), np.zeros(4))
    with pytest.raises(ValueError):
        pareto_front(np.ones((3, 2)), np.zeros(3))


# ---- ParetoOptimizer over the engine double ---------------------------------------------------------------------------------------
class EhviFakeEngine(FakeEngine):
    def overlapped_fits(self):
        import contextlib

        self.calls.append(("overlapped_fits",))
        return contextlib.nullcontext()

    def ehvi_argbest(self, levels, cell_lo, cell_hi, k_seeds=0, index_offset=0, return_values=False):
        self.calls.append(("ehvi_argbest", int(np.shape(cell_lo)[0]), k_seeds))
        rows = [np.asarray(r)[:int(np.argmax(np.isposinf(r))) + 1] for r in levels]
        m = len(rows)
        mu = np.stack([self.post[j][0] for j in range(m)])
        sd = np.stack([self.post[j][1] for j in range(m)])
        self.ehvi = T.ehvi_values(mu, sd, rows, cell_lo, cell_hi)
        bi, bv, si, sv = T.argbest(-self.ehvi, k_seeds, index_offset)
        return bi, bv, si, sv, (-self.ehvi if return_values else None)


BOUNDS = {"a": (0.0, 1.0), "b": (-1.0, 2.0), "c": (0.5, 1.5)}


def _objectives(X, m):
    f = [np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1]) + X[:, 2] ** 2, -((X[:, 0] - 0.7) ** 2) - 0.3 * X[:, 1] + 0.2 * X[:, 2],
         np.cos(2.0 * X[:, 2]) + 0.5 * X[:, 0]]
    return np.column_stack(f[:m])


def _optimizer(m=2, n=14, seed=3, engine=None, **kw):
    eng = EhviFakeEngine() if engine is None else engine
    opt = ParetoOptimizer(BOUNDS, m, np.full(m, -1.5), n_restarts_optimizer=2, random_state=seed, engine=eng, **kw)
    for gp in opt._gps:
        gp.lml_on_device = False
    lo, hi = np.array(list(BOUNDS.values())).T
    X = lo + np.random.RandomState(0).uniform(size=(n, 3)) * (hi - lo)
    for x, y in zip(X, _objectives(X, m)):
        opt.register(dict(zip(BOUNDS, x)), y)
    return opt, eng


@pytest.mark.parametrize("m", [2, 3])
def test_suggest_calls_randomstate_and_info(m):
    M = 500
    opt, eng = _optimizer(m)
    params, info = opt.suggest(n_random=M, return_info=True)
    names = [c[0] for c in eng.calls]
    # the call order: the m fits in slot order, ONE candidate draw, one posterior per slot in slot order, ehvi_argbest
    assert names[0] == "overlapped_fits"
    assert [c[1] for c in eng.calls if c[0] == "fit"] == list(range(m))
    assert names.count("generate_candidates_like") == 1 and [c[1] for c in eng.calls if c[0] == "posterior"] == list(range(m))
    last_fit = max(i for i, c in enumerate(names) if c in ("fit", "lml", "lml_batch"))
    assert last_fit < names.index("generate_candidates_like") < names.index("posterior") < names.index("ehvi_argbest")
    assert names[-1] == "ehvi_argbest" and names.count("ehvi_argbest") == 1
    assert not {"posterior_refresh", "fit_append", "polish_seeds", "predict_grad", "set_candidates", "acq_argbest"} & set(names)
    # the RandomState: the theta searches in slot order, then the candidate draw — a twin that does just that ends in the same state
    twin, teng = _optimizer(m)
    for j, gp in enumerate(twin._gps):
        gp.fit(twin.params, twin.targets[:, j])
    teng.generate_candidates_like(M, twin.bounds[:, 0], twin.bounds[:, 1], twin._random_state)
    assert B.same_state(opt._random_state, twin._random_state) and np.array_equal(eng.Xc, teng.Xc)
    assert all(gp.random_state is opt._random_state for gp in opt._gps)
    # the pick and the info
    front = pareto_front(opt.targets, opt.ref_point)
    assert set(info) == {"value", "index", "n_cells", "front_size"}
    assert info["front_size"] == front.shape[0] and info["n_cells"] == box_decomposition(front, opt.ref_point)[2].shape[0]
    assert isinstance(info["index"], int) and isinstance(info["value"], float) and info["value"] > 0.0
    assert info["index"] == int(eng.ehvi.argmax()) and info["value"] == eng.ehvi.max()
    assert list(params) == list(BOUNDS) and np.array_equal(np.array(list(params.values())), eng.Xc[info["index"]])
    again, _ = _optimizer(m)
    assert again.suggest(n_random=M) == params


def test_front_and_hypervolume_after_register():
    opt, _ = _optimizer(2, n=0)
    assert len(opt) == 0 and opt.hypervolume == 0.0 and opt.front[0].shape == (0, 3) and opt.front[1].shape == (0, 2)
    opt.register({"a": 0.1, "b": 0.0, "c": 1.0}, [0.0, 1.0])
    opt.register(np.array([0.2, 0.0, 1.0]), [1.0, 0.0])
    opt.register({"c": 1.0, "a": 0.3, "b": 0.0}, [0.5, 0.5])          # keys in another order
    opt.register({"a": 0.4, "b": 0.0, "c": 1.0}, [0.4, 0.4])          # dominated
    opt.register({"a": 0.5, "b": 0.0, "c": 1.0}, [1.0, 0.0])          # a duplicate: kept once, at its first observation
    opt.register({"a": 0.6, "b": 0.0, "c": 1.0}, [-1.5, 9.0])         # on the reference point's boundary: not above it
    X, Y = opt.front
    assert Y.tolist() == [[0.0, 1.0], [1.0, 0.0], [0.5, 0.5]] and X[:, 0].tolist() == [0.1, 0.2, 0.3]
    assert opt.hypervolume == pytest.approx(T.hv_brute(opt.targets, opt.ref_point), rel=1e-14)
    assert opt.hypervolume == pytest.approx(2.5 * 1.5 + 0.5 * 2.0 + 0.5 * 1.5, rel=1e-14)
    for bad in ({"a": 0.1, "b": 0.0}, np.zeros(2), {"a": np.nan, "b": 0.0, "c": 1.0}):
        with pytest.raises(ValueError, match="params"):
            opt.register(bad, [0.0, 0.0])
    for bad in ([0.0], [0.0, np.inf], [0.0, 0.0, 0.0]):
        with pytest.raises(ValueError, match="targets"):
            opt.register({"a": 0.1, "b": 0.0, "c": 1.0}, bad)
    assert len(opt) == 6


def test_refusals_and_their_order():
    from sklearn.gaussian_process.kernels import RationalQuadratic

    from bayesianoptimization_amd.engine import GroupEngine

    for bad in (0, 4, 2.0, True):
        with pytest.raises(ValueError, match="n_objectives"):
            ParetoOptimizer(BOUNDS, bad, np.zeros(2))
    with pytest.raises(ValueError, match="ref_point"):
        ParetoOptimizer(BOUNDS, 2, np.zeros(3))
    with pytest.raises(TypeError, match="unknown flags"):
        ParetoOptimizer(BOUNDS, 2, np.zeros(2), lml_on_device=False)
    # the argument check comes first, then the empty store — whatever else is wrong
    group = object.__new__(GroupEngine)
    group.__dict__.update(_g=None, _h=None)
    empty, eng = _optimizer(2, n=0, engine=group, kernel=RationalQuadratic())
    for bad in (0, -3, 1.5, True, None):
        with pytest.raises(ValueError, match="n_random"):
            empty.suggest(n_random=bad)
    with pytest.raises(A.TargetSpaceEmptyError, match="without previous samples"):
        empty.suggest()
    # ... then the device group, before the host-mode model
    opt, _ = _optimizer(2, engine=group, kernel=RationalQuadratic())
    with pytest.raises(NotImplementedError, match="device group"):
        opt.suggest()
    with pytest.raises(NotImplementedError, match="device group"):
        GroupEngine.ehvi_argbest(group, None, None, None)
    # ... then the host-mode model, before the front's size
    big_front = T.random_front(MAX_FRONT + 1, 2, seed=9)
    opt, eng = _optimizer(2, n=0, kernel=RationalQuadratic())
    for i, y in enumerate(big_front):
        opt.register([i / 200.0, 0.0, 1.0], y)
    with pytest.raises(NotImplementedError, match="objective 0's model runs on the host"):
        opt.suggest()
    assert not eng.calls
    # more than 128 points on the front: refused, never thinned, and nothing ran
    opt, eng = _optimizer(2, n=0)
    for i, y in enumerate(big_front):
        opt.register([i / 200.0, 0.0, 1.0], y)
    assert opt.front[1].shape[0] == MAX_FRONT + 1
    with pytest.raises(NotImplementedError, match="129 points"):
        opt.suggest(n_random=50)
    assert not eng.calls
    # 128 points are served
    opt, eng = _optimizer(2, n=0)
    for i, y in enumerate(big_front[:MAX_FRONT]):
        opt.register([i / 200.0, 0.0, 1.0], y)
    params, info = opt.suggest(n_random=50, return_info=True)
    assert info["front_size"] == 128 and info["n_cells"] == 129


def test_exported_and_header_limits():
    import bayesianoptimization_amd as pkg
    from bayesianoptimization_amd import multiobjective

    for name in ("ParetoOptimizer", "pareto_front", "hypervolume", "box_decomposition"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(multiobjective, name)
    hdr = open(os.path.join(ROOT, "include", "gpbo.h")).read()
    for name, value in (("OBJECTIVES", 3), ("LEVELS", 130), ("CELLS", 16641)):
        assert getattr(_lib, "MAX_EHVI_" + name) == value and re.search(rf"^#define GPBO_MAX_EHVI_{name}\s+{value}\b", hdr, flags=re.M)
    m = re.search(r"^int gpbo_ehvi_argbest\((.*?)\);", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), flags=re.M | re.S)
    assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES["gpbo_ehvi_argbest"][1]) == 14
    assert not [n for n in _lib.SIGNATURES if "ehvi" in n and n != "gpbo_ehvi_argbest"]      # no group / communicator form
    assert _lib.ABI_VERSION == 4 and re.search(r"^#define GPBO_ABI_VERSION 4\b", hdr, flags=re.M)
    build = open(os.path.join(ROOT, "bayesianoptimization_amd", "build.py")).read()
    assert re.search(r'"ehvi\.hip": \["-ffp-contract=off"\]', build)
