"""CPU: the trust-region suggest's host side — the NumPy restatement of the device generator (tests/turbo_truth.py) against SciPy's
own Sobol engine and against the definition's edge cases, the `TrustRegion` state machine and its box, and `suggest_turbo` over a
recording engine double: the refusal order, the RandomState draws, the design branch after a restart, the box a climb receives.
The device generator itself is checked in tests/test_gpu_turbo.py."""
import functools
import math
import os
import re
import warnings

import numpy as np
import pytest

import batch_truth as B
import paths_ascent_truth as PA
import turbo_truth as T
from bayesianoptimization_amd import TrustRegion, _lib, sobol_tables, suggest_turbo
from bayesianoptimization_amd import _suggest as S
from bayesianoptimization_amd import turbo
from conftest import ROOT


# ---- the truth against SciPy and against the definition ---------------------------------------------------------------------------
def test_philox_known_answers():
    """Random123's known-answer vectors for philox4x32-10."""
    got = [int(v[0]) for v in T.philox4x32_10([0], [0], [0], [0], 0)]
    assert got == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    ones = 0xFFFFFFFF
    got = [int(v[0]) for v in T.philox4x32_10([ones], [ones], [ones], [ones], (ones << 32) | ones)]
    assert got == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


@pytest.mark.parametrize("d", [1, 3, 16, 64])
@pytest.mark.parametrize("M", [1, 37, 1000])
def test_truth_sobol_points_equal_scipy(d, M):
    from scipy.stats import qmc

    seed = 1000 * d + M
    sv, shift = sobol_tables(d, seed)
    assert sv.dtype == np.uint32 and sv.shape == (d, 30) and shift.dtype == np.uint32 and shift.shape == (d,)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")              # (the balance warning: M is deliberately no power of two)
        want = qmc.Sobol(d, scramble=True, seed=seed).random(M)
    got = T.sobol_unit(M, sv, shift)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    # the assembly at threshold 2^32 over the unit box is the same matrix
    assert np.array_equal(T.generate(M, np.full(d, 0.5), np.zeros(d), np.ones(d), sv, shift, 2 ** 32, 77), want)


def test_sobol_tables_refuses_an_unknown_scipy(monkeypatch):
    from scipy.stats import qmc

    class Other(qmc.Sobol):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self._sv = self._sv.astype(np.uint64)

    monkeypatch.setattr(qmc, "Sobol", Other)
    with pytest.raises(NotImplementedError, match="scipy"):
        sobol_tables(3, 1)


def test_truth_mask_threshold_zero_one_fallback_column_per_row():
    mask = T.mask(4096, 16, 0, 12345)
    assert (mask.sum(axis=1) == 1).all()
    assert set(np.argmax(mask, axis=1).tolist()) == set(range(16))
    # another key, another pattern; d = 1: the one column
    assert not np.array_equal(mask, T.mask(4096, 16, 0, 12346))
    assert T.mask(9, 1, 0, 5).all()


def test_truth_mask_threshold_full_perturbs_everything():
    d, M = 16, 300
    sv, shift = sobol_tables(d, 4)
    centre = np.full(d, 0.123456789)                 # not on the Sobol grid (no multiple of 2^-30)
    X = T.generate(M, centre, np.full(d, -1.0), np.full(d, 2.0), sv, shift, 2 ** 32, 9)
    assert T.mask(M, d, 2 ** 32, 9).all() and not (X == centre).any()
    # in between: the share of perturbed coordinates follows the threshold, the others are the centre bit for bit
    mask = T.mask(4096, d, 2 ** 30, 9)
    assert abs(mask.mean() - 0.25) < 0.01
    X = T.generate(4096, centre, np.full(d, -1.0), np.full(d, 2.0), sv, shift, 2 ** 30, 9)
    assert np.array_equal(X == centre, ~mask) and (X >= -1.0).all() and (X < 2.0).all()


# ---- TrustRegion ------------------------------------------------------------------------------------------------------------------
def test_trust_region_counters_and_length():
    s = TrustRegion(8, 4)
    assert s.failure_tolerance == 2 and s.success_tolerance == 3 and s.length == 0.8 and s.best == -np.inf
    assert TrustRegion(3, 4).failure_tolerance == 1 and TrustRegion(20, 8).failure_tolerance == 3
    s.observe([])
    assert s.seen is None and s.successes == s.failures == 0
    s.observe([1.0, 0.5])                            # the first batch improves on -inf
    assert (s.successes, s.failures, s.best, s.seen, s.length) == (1, 0, 1.0, 2, 0.8)
    s.observe([1.0])                                 # equal to best: a failure
    assert (s.successes, s.failures, s.best) == (0, 1, 1.0)
    s.observe([1.0005])                              # within rel_improvement: a failure, the second -> halve; best still rises
    assert (s.successes, s.failures, s.length, s.best) == (0, 0, 0.4, 1.0005)
    for k, top in enumerate([2.0, 3.0]):
        s.observe([top, -5.0])
        assert (s.successes, s.failures, s.length) == (k + 1, 0, 0.4)
    s.observe([4.0])                                 # the third success in a row: double
    assert (s.successes, s.failures, s.length, s.best) == (0, 0, 0.8, 4.0)
    for top in (5.0, 6.0, 7.0):
        s.observe([top])
    assert s.length == 1.6
    for top in (8.0, 9.0, 10.0):
        s.observe([top])
    assert s.length == 1.6 and s.successes == 0      # capped at length_max
    s.observe([0.0])
    s.observe([11.0])                                # a success resets the failures
    assert (s.successes, s.failures) == (1, 0)
    # negative best: the margin is relative to |best|
    n = TrustRegion(2, 1, failure_tolerance=5)
    n.observe([-10.0])
    n.observe([-9.995])
    assert n.failures == 1 and n.best == -9.995
    n.observe([-9.9])
    assert n.successes == 1


def test_trust_region_restart():
    s = TrustRegion(4, 4, length=0.8, length_min=0.3)
    assert s.failure_tolerance == 1 and not s.design_pending and s.origin == 0 and s.restarts == 0
    s.observe([1.0, 2.0, 0.0, 0.5])
    s.observe([1.0] * 4)                             # 0.8 -> 0.4: still >= length_min
    assert (s.length, s.restarts, s.design_pending, s.origin) == (0.4, 0, False, 0)
    s.observe([1.5] * 4)                             # 0.4 -> 0.2 < 0.3: restart
    assert (s.length, s.restarts, s.design_pending, s.origin, s.seen) == (0.8, 1, True, 12, 12)
    assert (s.successes, s.failures, s.best) == (0, 0, -np.inf)
    s.observe([-3.0])                                # the first batch after the restart improves on -inf
    assert (s.successes, s.best, s.origin) == (1, -3.0, 12)


def test_trust_region_box():
    bounds = np.array([[0.0, 1.0], [-2.0, 2.0], [10.0, 12.0]])
    r = bounds[:, 1] - bounds[:, 0]
    s = TrustRegion(3, 2, length=0.2)
    ls = np.array([0.1, 1.6, 0.2])
    centre = np.array([0.5, 0.0, 11.0])
    lo, hi = s.box(centre, ls, bounds)
    side = hi - lo
    assert np.allclose(side / r / (ls / r), (side / r / (ls / r))[0], rtol=1e-14)          # proportional to the length scales
    assert math.isclose(float(np.prod(side)), 0.2 ** 3 * float(np.prod(r)), rel_tol=1e-13)
    assert np.allclose((lo + hi) / 2, centre, rtol=1e-14)
    # a scalar length scale is d equal ones (the GP's length scale is in the parameters' own units): by the formula the sides are
    # EQUAL, length * geomean(r) each, whatever the value — and proportional to r exactly where the space's sides are equal
    lo, hi = s.box(centre, 0.37, bounds)
    assert np.allclose(hi - lo, 0.2 * 2.0, rtol=1e-14)                        # geomean(1, 4, 2) = 2
    for other in (np.array([0.37]), np.full(3, 0.37), 5.0):
        lo1, hi1 = s.box(centre, other, bounds)
        assert np.allclose(lo, lo1, rtol=1e-14) and np.allclose(hi, hi1, rtol=1e-14)
    cube = np.array([[0.0, 4.0], [-2.0, 2.0], [10.0, 14.0]])
    lo, hi = s.box(np.array([2.0, 0.0, 12.0]), 0.37, cube)
    assert np.allclose(hi - lo, 0.2 * (cube[:, 1] - cube[:, 0]), rtol=1e-14)
    # the centre on a face: clipped to the bounds
    face = np.array([0.0, 2.0, 11.0])
    lo, hi = s.box(face, 0.37, bounds)
    assert lo[0] == 0.0 and math.isclose(hi[0], 0.2) and hi[1] == 2.0 and math.isclose(lo[1], 1.8) and (lo >= bounds[:, 0]).all()
    assert (hi <= bounds[:, 1]).all()


# ---- suggest_turbo over a recording engine double ----------------------------------------------------------------------------------
class TurboFakeEngine(PA.AscentFakeEngine):
    """paths_ascent_truth.AscentFakeEngine (TEST DOUBLE ONLY) + generate_candidates_trust_region by the truth; records the
    generator's arguments and the box of every climb."""

    def generate_candidates_trust_region(self, M, centre, lo, hi, sv, shift, bits, mask_threshold, mask_key):
        self.calls.append(("generate_candidates_trust_region", M))
        self.tr_args = dict(M=M, centre=np.array(centre), lo=np.array(lo), hi=np.array(hi), sv=sv, shift=shift, bits=bits,
                            threshold=mask_threshold, key=mask_key)
        self.Xc = T.generate(M, centre, lo, hi, sv, shift, mask_threshold, mask_key)
        self.n_candidates = M
        self.post = {}

    def ascend_paths(self, omega, phase, weights, eps, box_lo, box_hi, **kw):
        self.boxes = getattr(self, "boxes", []) + [(np.array(box_lo), np.array(box_hi))]
        return super().ascend_paths(omega, phase, weights, eps, box_lo, box_hi, **kw)


D, N, M = 3, 30, 600
_driver = functools.partial(B.suggest_driver, TurboFakeEngine, n_random=M)


def _replay_seeds(rng):
    return int(rng.randint(0, 2 ** 31 - 1)), int(rng.randint(0, 2 ** 63 - 1, dtype=np.int64))


@pytest.mark.parametrize("refine", [0, 2])
def test_draws_calls_and_box(refine):
    drv, eng, X, y = _driver()
    twin, teng, _, _ = _driver()
    state = TrustRegion(D, 5, length=0.4)
    picks = suggest_turbo(drv, 5, state, n_random=M, n_features=64, refine=refine, max_iter=20)
    assert (state.seen, state.best, state.successes, state.failures, state.length) == (N, y.max(), 0, 0, 0.4)
    # the replay: the fit, the two seeds, then the draws of the one group
    model = S.fit_model(twin._gp, twin._space, "twin")
    rng = twin._random_state
    seed, key = _replay_seeds(rng)
    centre = X[int(np.argmax(y))]
    ls = np.atleast_1d(twin._gp.kernel_.length_scale)
    lo, hi = TrustRegion(D, 5, length=0.4).box(centre, ls, B.SUGGEST_BOUNDS)
    a = eng.tr_args
    sv, shift = sobol_tables(D, seed)
    assert a["M"] == M and a["bits"] == 30 and a["key"] == key and a["threshold"] == 2 ** 32      # min(1, 20 / 3) = 1
    assert np.array_equal(a["centre"], centre) and np.array_equal(a["lo"], lo) and np.array_equal(a["hi"], hi)
    assert np.array_equal(a["sv"], sv) and np.array_equal(a["shift"], shift)
    teng.generate_candidates_trust_region(M, centre, lo, hi, sv, shift, 30, 2 ** 32, key)
    want = S.thompson_picks(twin._gp, twin._space, teng, rng, model, 5, 64, refine, 20, box=(lo, hi))
    assert picks == want and B.same_state(drv._random_state, twin._random_state)
    names = [c[0] for c in eng.calls]
    assert names.count("fit") == 1 and names.count("generate_candidates_trust_region") == 1
    assert names.index("fit") < names.index("generate_candidates_trust_region")
    assert not {"generate_candidates_like", "posterior", "set_candidates"} & set(names)
    rows = np.array([list(p.values()) for p in picks])
    assert (rows >= lo).all() and (rows <= hi).all() and list(picks[0]) == drv._space.keys
    if refine:
        assert names.count("ascend_paths") == 1 and "sample_paths" not in names
        assert len(eng.boxes) == 1 and np.array_equal(eng.boxes[0][0], lo) and np.array_equal(eng.boxes[0][1], hi)
        assert not np.array_equal(lo, B.SUGGEST_BOUNDS[:, 0])            # (the region is not the space)
    else:
        assert names.count("sample_paths") == 1 and "ascend_paths" not in names
        B.rows_to_indices(picks, eng.Xc)


def test_perturb_and_catching_up():
    drv, eng, X, y = _driver()
    state = TrustRegion(D, 2)
    suggest_turbo(drv, 2, state, n_random=64, n_features=16, perturb=0.25)
    assert eng.tr_args["threshold"] == 2 ** 30
    # the caller registers the results; the next call observes them
    drv._space.register(np.array([0.5, 0.5, 1.0]), float(y.max()) + 1.0)
    drv._space.register(np.array([0.6, 0.5, 1.0]), float(y.min()))
    suggest_turbo(drv, 2, state, n_random=64, n_features=16, perturb=1)
    assert (state.seen, state.successes, state.failures, state.best) == (N + 2, 1, 0, y.max() + 1.0)
    assert eng.tr_args["threshold"] == 2 ** 32 and np.array_equal(eng.tr_args["centre"], [0.5, 0.5, 1.0])
    suggest_turbo(drv, 2, state, n_random=64, n_features=16)              # nothing new: nothing observed
    assert (state.seen, state.successes, state.failures) == (N + 2, 1, 0)


def test_design_branch_after_a_restart():
    drv, eng, X, y = _driver()
    state = TrustRegion(D, 4)
    suggest_turbo(drv, 4, state, n_random=64, n_features=16)
    state.length, state.failures = state.length_min, state.failure_tolerance - 1
    for k in range(4):
        drv._space.register(np.array([0.1 * (k + 1), 0.0, 1.0]), float(y.min()) - 1.0)
    del eng.calls[:]
    before = drv._random_state.get_state()
    picks = suggest_turbo(drv, 4, state, n_random=64, n_features=16)
    assert (state.restarts, state.design_pending, state.origin, state.seen, state.length) == (1, False, N + 4, N + 4, 0.8)
    assert [c[0] for c in eng.calls] == ["generate_candidates_trust_region"]          # no fit, no sampling
    rng = np.random.RandomState(0)
    rng.set_state(before)
    seed, key = _replay_seeds(rng)
    assert B.same_state(rng, drv._random_state)                                        # the two seeds and nothing else
    a = eng.tr_args
    lo, hi = B.SUGGEST_BOUNDS[:, 0], B.SUGGEST_BOUNDS[:, 1]
    assert a["M"] == 4 and a["threshold"] == 2 ** 32 and a["key"] == key and np.array_equal(a["lo"], lo) and np.array_equal(a["hi"], hi)
    sv, shift = sobol_tables(D, seed)
    rows = np.array([list(p.values()) for p in picks])
    assert np.array_equal(rows, lo + (hi - lo) * T.sobol_unit(4, sv, shift))
    # the design is registered; the next call is an ordinary step centred on the best point SINCE the restart
    for k, x in enumerate(rows):
        drv._space.register(x, float(y.min()) - 10.0 - k)
    suggest_turbo(drv, 4, state, n_random=64, n_features=16)
    assert np.array_equal(eng.tr_args["centre"], rows[0]) and state.best == y.min() - 10.0 and state.successes == 1
    assert "fit" in [c[0] for c in eng.calls]


def test_refusals_and_their_order():
    drv, eng, X, y = _driver()
    ok = TrustRegion(D, 4)
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="q must be"):
            suggest_turbo(drv, bad, ok)
    for bad in (0, 2 ** 30 + 1):
        with pytest.raises(ValueError, match="n_random"):
            suggest_turbo(drv, 4, ok, n_random=bad)
    for bad in (0, 4097):
        with pytest.raises(ValueError, match="n_features"):
            suggest_turbo(drv, 4, ok, n_features=bad)
    for bad in (None, object(), TrustRegion(D + 1, 4), TrustRegion(D, 5)):
        with pytest.raises(ValueError, match="TrustRegion"):
            suggest_turbo(drv, 4, bad)
    for bad in (0, 0.0, -0.5, 1.5, True, "1"):
        with pytest.raises(ValueError, match="perturb"):
            suggest_turbo(drv, 4, ok, perturb=bad)
    for bad in (-1, 9, 1.5, True):
        with pytest.raises(ValueError, match="refine"):
            suggest_turbo(drv, 4, ok, refine=bad)
    assert not eng.calls and ok.seen is None
    # the caller's own checks come before the gate, the gate before refine
    bare = type("Bare", (), {"_gp": object(), "_space": None})()
    with pytest.raises(ValueError, match="q must be"):
        suggest_turbo(bare, 0, ok)
    drv2, _, _, _ = _driver()
    drv2._gp = object()
    with pytest.raises(ValueError, match="perturb"):
        suggest_turbo(drv2, 4, ok, perturb=2.0, refine=99)
    with pytest.raises(NotImplementedError, match="accelerate"):
        suggest_turbo(drv2, 4, ok, refine=99)
    group = B.check_shared_refusals(lambda d: suggest_turbo(d, 4, TrustRegion(D, 4)), _driver, "suggest_turbo")
    with pytest.raises(NotImplementedError, match="device group has no trust-region generator"):
        type(group).generate_candidates_trust_region(group, 1, [0.5], [0.0], [1.0], None, None, 30, 0, 0)
    # an engine without the generator, and one without the ascent
    drv, eng, X, y = _driver()
    drv._gp.engine = PA.AscentFakeEngine()
    with pytest.raises(NotImplementedError, match="sample_paths / generate_candidates_trust_region"):
        suggest_turbo(drv, 4, ok)

    class NoAscent(TurboFakeEngine):
        ascend_paths = property()

    drv, eng, X, y = B.suggest_driver(NoAscent, n_random=M)
    with pytest.raises(NotImplementedError, match="ascend_paths"):
        suggest_turbo(drv, 4, ok, refine=1)
    assert ok.seen is None


def test_engine_method_checks_its_arguments_on_the_host():
    from bayesianoptimization_amd.engine import GpEngine

    eng = object.__new__(GpEngine)                   # (no context: every case is refused before the library is reached)
    sv, shift = sobol_tables(3, 1)
    c, lo, hi = np.full(3, 0.5), np.zeros(3), np.ones(3)
    cases = [((8, c[:2], lo, hi, sv, shift, 30, 0, 0), "one length"), ((8, c, lo[:2], hi, sv, shift, 30, 0, 0), "one length"),
             ((8, np.zeros((3, 1)), lo, hi, sv, shift, 30, 0, 0), "one length"),
             ((8, c, lo, hi, sv.astype(np.int64), shift, 30, 0, 0), "uint32"), ((8, c, lo, hi, sv, shift.astype(np.float64), 30, 0, 0), "uint32"),
             ((8, c, lo, hi, sv[:, :29], shift, 30, 0, 0), r"\(d, bits\)"), ((8, c, lo, hi, sv, shift[:2], 30, 0, 0), r"\(d, bits\)"),
             ((8, c, lo, hi, sv, shift, 30.0, 0, 0), "bits"), ((8, c, lo, hi, sv, shift, 30, -1, 0), "mask_threshold"),
             ((8, c, lo, hi, sv, shift, 30, 2 ** 32 + 1, 0), "mask_threshold")]
    for args, match in cases:
        with pytest.raises(ValueError, match=match):
            eng.generate_candidates_trust_region(*args)


# ---- header and bindings ----------------------------------------------------------------------------------------------------------
def test_exported_and_bound():
    import bayesianoptimization_amd as pkg

    for name in ("suggest_turbo", "TrustRegion", "sobol_tables"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(turbo, name)
    hdr = open(os.path.join(ROOT, "include", "gpbo.h")).read()
    m = re.search(r"^int gpbo_generate_candidates_trust_region\((.*?)\);", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), flags=re.M | re.S)
    assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES["gpbo_generate_candidates_trust_region"][1]) == 11
    bound = [n for n in list(_lib.SIGNATURES) + list(_lib.DEBUG_SIGNATURES) if "trust_region" in n]
    assert bound == ["gpbo_generate_candidates_trust_region"]                   # no group / communicator form
    assert _lib.ABI_VERSION == 4 and "#define GPBO_ABI_VERSION 4" in hdr
    # the Philox round function exists once, in the header both generators include
    csrc = os.path.join(ROOT, "bayesianoptimization_amd", "csrc")
    holders = sorted(f for f in os.listdir(csrc) if "0xD2511F53" in open(os.path.join(csrc, f)).read())
    assert holders == ["philox.h"]
    for f in ("candidates.hip", "trust_region.hip"):
        assert '#include "philox.h"' in open(os.path.join(csrc, f)).read()
