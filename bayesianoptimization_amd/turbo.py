"""suggest_turbo(optimizer, q, state) — q points to probe in parallel by trust-region Bayesian optimisation (TuRBO-1; Eriksson,
Pearce, Gardner, Turner & Poloczek, NeurIPS 2019, "Scalable global optimization via local Bayesian optimization").

With thousands of observations in tens of dimensions one global model does not search the whole box well: its candidates are
spread over a volume no candidate count fills.  TuRBO keeps a box around the incumbent — the TRUST REGION, side lengths
proportional to the GP's length scales —, draws the candidates inside it by changing only a FEW coordinates of the incumbent (a
scrambled Sobol point in those, the incumbent's value in the others), picks the batch by Thompson sampling, and doubles or halves
the box by whether the batch improved; a box that has shrunk below its minimum is abandoned and the search restarts.

The candidates are generated on the device (the engine's `generate_candidates_trust_region`, gpbo_generate_candidates_trust_region;
include/gpbo.h has the definition of an element): no host sampling, no upload.  The draws and the picks are `suggest_thompson`'s
(thompson.py) over those candidates.  The state lives in a `TrustRegion` the caller keeps; the caller only registers results.
"""
from __future__ import annotations

import math

import numpy as np

from . import _suggest as S
from ._lib import MAX_PATH_FEATURES as MAX_FEATURES, MAX_PATH_STARTS as MAX_STARTS

SOBOL_BITS = 30            # scipy.stats.qmc.Sobol's default: 2^30 points
MAX_CANDIDATES = 2 ** SOBOL_BITS


def sobol_tables(d: int, seed, bits: int = SOBOL_BITS):
    """(sv (d, bits) uint32, shift (d,) uint32): the scrambled direction numbers and the digital shift of
    `scipy.stats.qmc.Sobol(d, scramble=True, seed=seed, bits=bits)` — point m of that sequence is, per column t,
    (shift[t] XOR over the set bits b of m ^ (m >> 1) of sv[t, b]) 2^-bits (tests/test_turbo_host.py checks that against
    `.random`).  SciPy keeps the tables in private attributes; where they are absent or of another kind: NotImplementedError."""
    import scipy
    from scipy.stats import qmc

    engine = qmc.Sobol(int(d), scramble=True, seed=seed, bits=int(bits))
    sv, shift = getattr(engine, "_sv", None), getattr(engine, "_shift", None)
    ok = (isinstance(sv, np.ndarray) and isinstance(shift, np.ndarray) and sv.dtype == np.uint32 and shift.dtype == np.uint32
          and sv.shape == (int(d), int(bits)) and shift.shape == (int(d),))
    if not ok:
        raise NotImplementedError(f"sobol_tables: scipy {scipy.__version__}'s qmc.Sobol does not keep its direction numbers and "
                                  f"shift as uint32 arrays _sv (d, bits) / _shift (d,)")
    return np.ascontiguousarray(sv).copy(), np.ascontiguousarray(shift).copy()


class TrustRegion:
    """The state of one trust region over a d-dimensional space probed q points at a time.  `length` is the region's base side as a
    fraction of the space's (before the length scales shape it).  Public state: `length`, `successes`, `failures` (consecutive
    improving / failing batches since the last change of length), `best` (the best target since `origin`), `restarts`, `seen` (the
    observations taken into account; None before the first), `origin` (the observation the current region started at: the centre is
    the best point from there on), `design_pending` (a restart happened and its initial design has not been suggested yet)."""

    def __init__(self, d: int, q: int, length: float = 0.8, length_min: float = 0.5 ** 7, length_max: float = 1.6,
                 success_tolerance: int = 3, failure_tolerance=None, rel_improvement: float = 1e-3):
        self.d = S.count(d, 1, None, "d must be an integer >= 1")
        self.q = S.count(q, 1, None, "q must be an integer >= 1")
        self.length_init, self.length_min, self.length_max = float(length), float(length_min), float(length_max)
        if not 0.0 < self.length_min <= self.length_init <= self.length_max:
            raise ValueError("need 0 < length_min <= length <= length_max")
        self.success_tolerance = S.count(success_tolerance, 1, None, "success_tolerance must be an integer >= 1")
        if failure_tolerance is None:
            failure_tolerance = math.ceil(max(4.0 / self.q, self.d / self.q))
        self.failure_tolerance = S.count(failure_tolerance, 1, None, "failure_tolerance must be an integer >= 1")
        self.rel_improvement = float(rel_improvement)
        self.length = self.length_init
        self.successes = self.failures = 0
        self.best = -np.inf
        self.restarts = 0
        self.seen = None
        self.origin = 0
        self.design_pending = False

    def observe(self, targets):
        """Take one batch of results into account (an empty batch: nothing happens).  The batch IMPROVES iff max(targets) > best +
        rel_improvement |best| (with best = -inf it does; a batch equal to best does not).  Improved: successes += 1, failures = 0;
        else successes = 0, failures += 1.  successes == success_tolerance: length = min(2 length, length_max), successes = 0;
        otherwise failures == failure_tolerance: length /= 2, failures = 0.  Then best = max(best, max(targets)).  length <
        length_min: RESTART — restarts += 1, length back to its initial value, both counters 0, best = -inf, origin = the number of
        observations seen so far, design_pending = True."""
        targets = np.asarray(targets, dtype=np.float64).ravel()
        if targets.size == 0:
            return
        top = float(targets.max())
        improved = self.best == -np.inf or top > self.best + self.rel_improvement * abs(self.best)
        if improved:
            self.successes, self.failures = self.successes + 1, 0
        else:
            self.successes, self.failures = 0, self.failures + 1
        if self.successes == self.success_tolerance:
            self.length, self.successes = min(2.0 * self.length, self.length_max), 0
        elif self.failures == self.failure_tolerance:
            self.length, self.failures = self.length / 2.0, 0
        self.best = max(self.best, top)
        self.seen = (self.seen or 0) + int(targets.size)
        if self.length < self.length_min:
            self.restarts += 1
            self.length = self.length_init
            self.successes = self.failures = 0
            self.best = -np.inf
            self.origin = self.seen
            self.design_pending = True

    def box(self, centre, length_scales, bounds):
        """(lo, hi) of the region around `centre`: with r the space's side lengths and l~ = length_scales / r (a scalar length scale
        is broadcast), the weights w = l~ / geomean(l~) and  lo = max(bounds_lo, centre - w length r / 2),  hi = min(bounds_hi,
        centre + w length r / 2): sides proportional to the length scales, of volume (length)^d prod r where nothing clips."""
        bounds = np.asarray(bounds, dtype=np.float64)
        centre = np.asarray(centre, dtype=np.float64).ravel()
        r = bounds[:, 1] - bounds[:, 0]
        scaled = np.broadcast_to(np.asarray(length_scales, dtype=np.float64).ravel(), r.shape) / r
        w = scaled / np.exp(np.mean(np.log(scaled)))
        half = w * self.length * r / 2.0
        return np.maximum(bounds[:, 0], centre - half), np.minimum(bounds[:, 1], centre + half)


def _sobol_seeds(rng):
    """The two draws of a candidate set, in this order: the Sobol scramble's seed, the mask's Philox key."""
    seed = rng.randint(0, 2 ** 31 - 1)
    key = rng.randint(0, 2 ** 63 - 1, dtype=np.int64)
    return int(seed), int(key)


def suggest_turbo(optimizer, q: int, state: TrustRegion, n_random: int = 10_000, n_features: int = 1024, refine: int = 0,
                  max_iter=None, perturb=None):
    """q parameter dicts to probe side by side, as `suggest_thompson` returns them; `optimizer` has been `accelerate()`d and
    `state` is the caller's `TrustRegion(d, q)`, the same object on every call.  The caller evaluates the points and registers the
    results; there is no separate update call.  In this order:

      1. the checks below, `suggest_thompson`'s refusals among them in its order.  The acquisition policy is neither consulted nor
         advanced.
      2. `state` catches up with the space: on its first use seen = len(space), best = the best target (the counters are untouched);
         afterwards `state.observe(space.target[seen:])`.
      3. if a restart is pending (`state.design_pending`, or nothing has been registered since `state.origin`): the two draws of
         step 5, then min(n_random, q) rows over the WHOLE space with every coordinate a Sobol point are generated on the device,
         the first q rows are returned (row i mod the count where n_random < q) and `design_pending` is cleared.  No fit, no sampling.
      4. `gp.fit` on ALL the data, theta search (and its RandomState draws) included.  The centre is the best point among those
         registered since `state.origin`, the region `state.box(centre, the GP's length scales, space.bounds)`.  (The paper
         discards the data at a restart; here the model keeps every observation — only the centre and `best` forget.)
      5. `seed = rng.randint(0, 2**31 - 1)`, then `key = rng.randint(0, 2**63 - 1, dtype=np.int64)` from the optimizer's
         RandomState; `sobol_tables(d, seed)`; `n_random` candidates generated on the device: the centre with each coordinate
         replaced, with probability `perturb` (None: min(1, 20 / d)) under the Philox key `key`, by the row's Sobol point in the region.
      6. ceil(q / 16) `sample_paths` calls (`refine=K`: `ascend_paths`, the climb confined to the REGION) with the draws of
         `suggest_thompson`'s step 4 per call, and its pick assembly.
    Afterwards `gp.predict` answers for the real data as before; slot 0 holds the fit of step 4.

    ValueError: q not an integer >= 1, n_random outside [1, 2^30], n_features outside [1, 4096], `state` not a TrustRegion of the
    space's dimension and this q, `perturb` not None or a number in (0, 1], refine not an integer in [0, 8].  TargetSpaceEmptyError on
    an empty space, ConstraintNotSupportedError with a constraint.  NotImplementedError, never a host fallback, for: a GP that is not
    on the engine's slot 0, a space with an input transform (int / categorical parameters), a model in host mode, a device group."""
    q = S.count(q, 1, None, "q must be an integer >= 1", "q must be >= 1")
    n_random, n_features = int(n_random), int(n_features)
    if not 1 <= n_random <= MAX_CANDIDATES:
        raise ValueError(f"n_random must be in [1, 2^{SOBOL_BITS}]")
    if not 1 <= n_features <= MAX_FEATURES:
        raise ValueError(f"n_features must be in [1, {MAX_FEATURES}]")
    d = int(optimizer._space.bounds.shape[0]) if getattr(optimizer, "_space", None) is not None else None
    if not isinstance(state, TrustRegion) or (d is not None and state.d != d) or state.q != q:
        raise ValueError("state must be a TrustRegion(d, q) of the space's dimension and this q")
    if perturb is not None:
        if isinstance(perturb, bool) or not isinstance(perturb, (int, float, np.integer, np.floating)) or not 0.0 < perturb <= 1.0:
            raise ValueError("perturb must be None or a number in (0, 1]")
    gp, space, eng = S.gate(optimizer, "suggest_turbo", "sampled", ("sample_paths", "generate_candidates_trust_region"),
                            "a device group has no path sampler; use a single device")
    refine = S.count(refine, 0, MAX_STARTS, f"refine must be an integer in [0, {MAX_STARTS}]")
    if refine and not hasattr(eng, "ascend_paths"):
        raise NotImplementedError("suggest_turbo: the engine has no ascend_paths")
    rng = optimizer._random_state
    probability = min(1.0, 20.0 / d) if perturb is None else float(perturb)

    if state.seen is None:
        state.seen, state.best = len(space), float(np.max(space.target))
    else:
        state.observe(space.target[state.seen:])
        state.seen = len(space)

    lo, hi = space.bounds[:, 0], space.bounds[:, 1]
    if state.design_pending or state.origin >= len(space):
        seed, key = _sobol_seeds(rng)
        sv, shift = sobol_tables(d, seed)
        n_rows = min(n_random, q)
        eng.generate_candidates_trust_region(n_rows, 0.5 * (lo + hi), lo, hi, sv, shift, SOBOL_BITS, 2 ** 32, key)
        rows = np.asarray(eng.get_candidate_rows(np.arange(q, dtype=np.int64) % n_rows, d), dtype=np.float64)
        state.design_pending = False
        return [space.array_to_params(x) for x in rows]

    model = S.fit_model(gp, space, "suggest_turbo")
    centre = np.asarray(space.params[state.origin:][int(np.argmax(space.target[state.origin:]))], dtype=np.float64)
    box = state.box(centre, gp._describe(gp.kernel_).length_scale, space.bounds)
    seed, key = _sobol_seeds(rng)
    sv, shift = sobol_tables(d, seed)
    eng.generate_candidates_trust_region(n_random, centre, box[0], box[1], sv, shift, SOBOL_BITS,
                                         min(2 ** 32, int(probability * 2 ** 32)), key)
    return S.thompson_picks(gp, space, eng, rng, model, q, n_features, refine, max_iter, box=box)
