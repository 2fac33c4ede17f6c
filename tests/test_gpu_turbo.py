"""GPU (-m gpu): gpbo_generate_candidates_trust_region — the trust-region candidate generator — BIT FOR BIT against its NumPy
restatement (tests/turbo_truth.py, itself checked against SciPy in tests/test_turbo_host.py) and against SciPy's Sobol engine, the
state the call leaves behind and every refusal, and `suggest_turbo` on the real engine: one step replayed by hand, and a short loop.

The generator's shapes are the smallest that reach every path: a row narrower than (d = 1, 3), equal to (d = 64: 16 lanes is the
widest ballot group) and not dividing a wave (d = 17), the ballot kernel (d = 16, 64) and the LDS kernel (d = 1, 3, 17), a Philox quad
that straddles two rows (d = 3, 17), one workgroup with a ragged tail and more than one workgroup (M = 255 / 257 / 4099), a Gray code
with a bit above 16 (M = 65 539).  The other row widths of the ballot kernel (d = 4, 8, 32: ballot groups of 1, 2 and 8 lanes) are
tests/test_gpu_instances.py's."""
import numpy as np
import pytest

import batch_truth as B
import turbo_truth as T
from bayesianoptimization_amd import TrustRegion, _lib, sobol_tables, suggest_turbo
from bayesianoptimization_amd import _suggest as S
from bayesianoptimization_amd import fused_acquisition as A
from bayesianoptimization_amd.engine import MATERN25, GroupEngine
from bayesianoptimization_amd.thompson import spectral_draw

pytestmark = pytest.mark.gpu

KEY = 0x1234567_89ABCDEF          # both key words in use
FULL = 2 ** 32


def read_all(eng, M, d):
    return np.vstack([eng.get_candidate_rows(np.arange(i, min(i + 4096, M)), d) for i in range(0, M, 4096)])


def box_of(d):
    """an asymmetric box with a negative lo, and a centre that is no Sobol grid point of it"""
    t = np.arange(d, dtype=np.float64)
    lo, hi = -1.5 - 0.01 * t, 0.75 + 0.1 * t
    return lo + (hi - lo) * (0.3137 + 0.001 * t) + 1e-11, lo, hi


SHAPES = [(d, M) for d in (1, 3, 16, 17, 64) for M in (1, 255, 257, 4099)] + [(16, 65539)]


@pytest.mark.parametrize("d,M", SHAPES, ids=[f"d{d}-m{M}" for d, M in SHAPES])
def test_generator_equals_the_truth_bit_for_bit(engine, d, M):
    centre, lo, hi = box_of(d)
    sv, shift = sobol_tables(d, 100 * d + M % 97)
    for threshold in dict.fromkeys((0, FULL, min(FULL, int(20 / d * 2 ** 32)), 2 ** 31)):      # (20 / d clips to 2^32 up to d = 20)
        engine.generate_candidates_trust_region(M, centre, lo, hi, sv, shift, 30, threshold, KEY)
        assert engine.n_candidates == M
        got = read_all(engine, M, d)
        want = T.generate(M, centre, lo, hi, sv, shift, threshold, KEY)
        same = got.view(np.uint64) == want.view(np.uint64)
        assert same.all(), (threshold, int((~same).sum()), np.argwhere(~same)[:4].tolist())
        changed = (got != centre).sum(axis=1)
        assert (changed >= 1).all()
        if threshold == 0:
            assert (changed == 1).all()
        if threshold == FULL:
            assert (changed == d).all()


def test_generator_equals_scipy_over_the_unit_box(engine):
    import warnings

    from scipy.stats import qmc

    d, M, seed = 16, 1000, 424242
    sv, shift = sobol_tables(d, seed)
    engine.generate_candidates_trust_region(M, np.full(d, 0.5), np.zeros(d), np.ones(d), sv, shift, 30, FULL, KEY)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = qmc.Sobol(d, scramble=True, seed=seed).random(M)
    assert np.array_equal(read_all(engine, M, d).view(np.uint64), want.view(np.uint64))


def test_other_bit_counts(engine):
    """bits = 32 (every bit of the word in use, M up to 2^32 allowed) and a short sequence that M fills exactly (M = 2^bits)."""
    d = 5
    centre, lo, hi = box_of(d)
    rng = np.random.RandomState(5)
    for bits, M in ((32, 1000), (7, 128), (1, 2)):
        sv = rng.randint(0, 2 ** bits, size=(d, bits), dtype=np.uint64).astype(np.uint32)
        shift = rng.randint(0, 2 ** bits, size=d, dtype=np.uint64).astype(np.uint32)
        engine.generate_candidates_trust_region(M, centre, lo, hi, sv, shift, bits, 2 ** 31, KEY)
        want = T.generate(M, centre, lo, hi, sv, shift, 2 ** 31, KEY)
        assert np.array_equal(read_all(engine, M, d).view(np.uint64), want.view(np.uint64)), bits


def test_state_after_the_call_and_every_refusal(engine):
    d, N, M = 3, 40, 300
    rs = np.random.RandomState(17)
    X, yn = rs.uniform(size=(N, d)), rs.standard_normal(N)
    engine.fit(X, yn, MATERN25, np.array([0.4]), 1e-4)
    # a posterior over OTHER candidates is resident when the generator runs: it must not survive
    engine.set_candidates(rs.uniform(size=(M, d)))
    stale = engine.posterior()
    centre, lo, hi = np.full(d, 0.4), np.full(d, 0.1), np.full(d, 0.9)
    sv, shift = sobol_tables(d, 3)
    engine.generate_candidates_trust_region(M, centre, lo, hi, sv, shift, 30, 2 ** 31, KEY)
    mu, sd = engine.posterior()
    rows = read_all(engine, M, d)
    engine.set_candidates(rows)
    mu2, sd2 = engine.posterior()
    assert np.array_equal(mu, mu2) and np.array_equal(sd, sd2) and not np.array_equal(mu, stale[0])
    # every refusal: ValueError, the resident candidates and their count as before
    engine.generate_candidates_trust_region(M, centre, lo, hi, sv, shift, 30, 2 ** 31, KEY)
    u32 = lambda a: a.ctypes.data_as(_lib.C.POINTER(_lib.C.c_uint32))          # noqa: E731
    from bayesianoptimization_amd._lib import dptr

    call = engine._lib.gpbo_generate_candidates_trust_region
    good = [engine._h, M, d, dptr(centre), dptr(lo), dptr(hi), u32(sv), 30, u32(shift), 2 ** 31, KEY]
    for k in (3, 4, 5, 6, 8):
        args = list(good)
        args[k] = None
        assert call(*args) == _lib.ERR_INVALID, k
    nan, inf = np.array([0.4, np.nan, 0.4]), np.array([0.9, np.inf, 0.9])
    sv32, sh32 = np.zeros((d, 32), np.uint32), shift
    bad = [dict(M=0), dict(M=-5), dict(M=2 ** 30 + 1), dict(sv=sv[:, :4].copy(), bits=4, M=17), dict(centre=nan), dict(lo=nan),
           dict(hi=inf), dict(lo=np.array([0.1, 0.95, 0.1])), dict(sv=np.zeros((d, 33), np.uint32), bits=33),
           dict(sv=np.zeros((d, 0), np.uint32), bits=0)]
    for change in bad:
        kw = dict(M=M, centre=centre, lo=lo, hi=hi, sv=sv, shift=shift, bits=30, mask_threshold=2 ** 31, mask_key=KEY)
        kw.update(change)
        with pytest.raises(ValueError, match="generate_candidates_trust_region"):
            engine.generate_candidates_trust_region(**kw)
    assert call(*(good[:9] + [2 ** 32 + 1, KEY])) == _lib.ERR_INVALID                  # (the engine refuses this one on the host)
    assert call(*(good[:1] + [1, 65] + good[3:])) == _lib.ERR_INVALID and call(*(good[:1] + [1, 0] + good[3:])) == _lib.ERR_INVALID
    assert call(engine._h, 2 ** 32 + 1, d, dptr(centre), dptr(lo), dptr(hi), u32(sv32), 32, u32(sh32), 0, KEY) == _lib.ERR_INVALID
    assert engine.n_candidates == M and np.array_equal(read_all(engine, M, d), rows)
    mu3, sd3 = engine.posterior()
    assert np.array_equal(mu3, mu) and np.array_equal(sd3, sd)
    # a valid call afterwards works; lo == hi and a centre outside the box are valid
    flat = np.array([0.1, 0.5, 0.9])
    engine.generate_candidates_trust_region(33, np.array([5.0, 5.0, 5.0]), flat, flat, sv, shift, 30, FULL, KEY)
    assert engine.n_candidates == 33 and np.array_equal(read_all(engine, 33, d), np.broadcast_to(flat, (33, d)))
    with pytest.raises(NotImplementedError, match="device group"):
        GroupEngine.generate_candidates_trust_region(object.__new__(GroupEngine), 1, centre, lo, hi, sv, shift, 30, 0, 0)


# ---- suggest_turbo on the real engine ---------------------------------------------------------------------------------------------
D, N, M, FEATURES = 6, 40, 4096, 256
BOUNDS = np.array([[0.0, 1.0], [-1.0, 2.0], [0.5, 1.5], [-3.0, -1.0], [0.0, 10.0], [-0.5, 0.5]])


def data():
    rs = np.random.RandomState(130)
    X = BOUNDS[:, 0] + rs.uniform(size=(N, D)) * (BOUNDS[:, 1] - BOUNDS[:, 0])
    U = (X - BOUNDS[:, 0]) / (BOUNDS[:, 1] - BOUNDS[:, 0])
    return X, np.sin(3.0 * U[:, 0]) * np.cos(2.0 * U[:, 1]) + U[:, 2] ** 2 - (U[:, 3:] - 0.4).sum(axis=1) ** 2


def driver(engine):
    X, y = data()
    return B.Driver(engine, X, y, BOUNDS, A.UpperConfidenceBound(kappa=2.576), seed=7, n_random=M)


def rows_of(picks):
    return np.array([list(p.values()) for p in picks])


@pytest.mark.parametrize("q", [5, 17])
def test_suggest_turbo_replayed_by_hand(engine, q):
    X, y = data()
    drv, twin, third = driver(engine), driver(engine), driver(engine)
    drv._gp.fit(X, y)
    state = TrustRegion(D, q, length=0.4)
    picks = suggest_turbo(drv, q, state, n_random=M, n_features=FEATURES)
    after = drv._gp.predict(X, return_std=True)         # the real data's model: what a plain fit in the call's place answers (below)
    assert (state.seen, state.best, state.successes, state.failures, state.length) == (N, y.max(), 0, 0, 0.4)
    assert len(picks) == q and list(picks[0]) == drv._space.keys and drv._acquisition_function.i == 0
    rows = rows_of(picks)
    # the region, recomputed from the state and the fitted length scales
    gp = drv._gp
    centre = X[int(np.argmax(y))]
    lo, hi = TrustRegion(D, q, length=0.4).box(centre, np.array(gp._ls), BOUNDS)
    assert (rows >= lo).all() and (rows <= hi).all() and (rows >= BOUNDS[:, 0]).all() and (rows <= BOUNDS[:, 1]).all()
    assert ((rows != centre).sum(axis=1) >= 1).all()
    assert (hi - lo < BOUNDS[:, 1] - BOUNDS[:, 0]).any()
    # the same engine calls by hand, from a twin RandomState
    twin._gp.fit(X, y)
    model = S.fit_model(twin._gp, twin._space, "twin")
    plain = twin._gp.predict(X, return_std=True)
    assert np.array_equal(after[0], plain[0]) and np.array_equal(after[1], plain[1]) and gp.X_train_.shape[0] == N
    rng = twin._random_state
    seed = rng.randint(0, 2 ** 31 - 1)
    key = rng.randint(0, 2 ** 63 - 1, dtype=np.int64)
    sv, shift = sobol_tables(D, seed)
    assert np.array_equal(np.array(twin._gp._ls), np.array(gp._ls))
    engine.generate_candidates_trust_region(M, centre, lo, hi, sv, shift, 30, FULL, int(key))       # min(1, 20 / 6) = 1
    index = []
    for first in range(0, q, 16):
        n = min(16, q - first)
        omega, phase = spectral_draw(twin._gp._kind, FEATURES, D, rng)
        w = rng.standard_normal((n, FEATURES))
        eps = rng.standard_normal((n, N)) * np.sqrt(model.noise)
        twin._gp._ensure_resident()
        index.extend(int(i) for i in engine.sample_paths(omega, phase, w, eps, y_mean=model.y_mean, y_std=model.y_std)[0])
    want = engine.get_candidate_rows(np.array(index), D)
    assert np.array_equal(rows.view(np.uint64), want.view(np.uint64))
    assert B.same_state(drv._random_state, rng)
    # refine: inside the region, the RandomState in the same place
    third._gp.fit(X, y)
    climbed = rows_of(suggest_turbo(third, q, TrustRegion(D, q, length=0.4), n_random=M, n_features=FEATURES, refine=2))
    assert climbed.shape == (q, D) and (climbed >= lo).all() and (climbed <= hi).all()
    assert B.same_state(third._random_state, rng)


def test_a_short_loop_and_a_forced_restart(engine):
    d, q, rounds = 8, 4, 10
    bounds = np.array([[-2.0, 3.0]] * d)

    def f(x):
        return -float(np.sum(np.asarray(x) ** 2))

    rs = np.random.RandomState(3)
    X = rs.uniform(-2.0, 3.0, size=(12, d))
    drv = B.Driver(engine, X, np.array([f(x) for x in X]), bounds, A.UpperConfidenceBound(kappa=2.576), seed=11, n_random=2048,
                   n_restarts_optimizer=1)
    state, shadow = TrustRegion(d, q), TrustRegion(d, q)
    shadow.seen, shadow.best = 12, float(drv._space.target.max())
    best_seen = [state.best]
    for r in range(rounds):
        picks = suggest_turbo(drv, q, state, n_random=2048, n_features=128)
        if r:
            shadow.observe(batch)
        assert (state.length, state.successes, state.failures, state.best, state.seen, state.restarts) == \
            (shadow.length, shadow.successes, shadow.failures, shadow.best, shadow.seen, shadow.restarts), r
        best_seen.append(state.best)
        batch = [f(list(p.values())) for p in picks]
        for p, t in zip(picks, batch):
            drv._space.register(np.array(list(p.values())), t)
    print(f"best per round {best_seen[1:]} final length {state.length}")
    assert state.restarts == 0 and all(b >= a for a, b in zip(best_seen[1:], best_seen[2:]))
    assert state.best > best_seen[1], "ten trust-region rounds found nothing better than the initial design on a sphere"
    # forced to the minimum by hand: the next failing batch restarts, the call returns a Sobol design over the whole space
    state.observe(batch)
    assert state.seen == len(drv._space)
    state.length, state.failures, state.successes = state.length_min, state.failure_tolerance - 1, 0
    worse = min(batch) - 1.0
    for k in range(q):
        drv._space.register(np.full(d, 2.5 - 0.1 * k), worse)
    n = len(drv._space)
    design = rows_of(suggest_turbo(drv, q, state, n_random=2048, n_features=128))
    assert (state.restarts, state.design_pending, state.origin, state.length, state.best) == (1, False, n, 0.8, -np.inf)
    assert design.shape == (q, d) and (design >= bounds[:, 0]).all() and (design < bounds[:, 1]).all()
    assert len({tuple(x) for x in design}) == q and engine.n_candidates == q
