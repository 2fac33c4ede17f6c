"""suggest_constrained_thompson(optimizer, q) and suggest_scbo(optimizer, q, state) — sampled batches for a CONSTRAINED space (SCBO;
Eriksson & Poloczek, AISTATS 2021, "Scalable constrained Bayesian optimization").

Thompson sampling with constraints draws one function from the posterior of the objective and one from each constraint over ONE
candidate set; a draw's pick is the best objective value among the candidates its constraint draws call feasible, and where none
is, the candidate of least total violation.  The engine's `sample_paths_constrained` (gpbo_sample_paths_constrained; include/gpbo.h
has the rule) does that for 16 draws at once without any of the (1 + C) x 16 x M values leaving the device.  `suggest_scbo` runs it
inside a TuRBO trust region (turbo.py) centred on the best FEASIBLE point, whose state — a `ConstrainedTrustRegion` — also counts a
batch that only reduces the violation as a success while nothing feasible is known.

There is no `refine`: a climbed draw can leave the feasible set.
"""
from __future__ import annotations

import contextlib
import warnings

import numpy as np

from . import _suggest as S
from ._lib import MAX_PATH_FEATURES as MAX_FEATURES, MAX_PATHS
from .thompson import spectral_draw
from .turbo import MAX_CANDIDATES, SOBOL_BITS, TrustRegion, _sobol_seeds, sobol_tables


def violation(values, lb, ub, std):
    """Total violation per row of constraint values (n, C) (or (n,) with one constraint): sum_j max(lb_j - c_j, c_j - ub_j, 0) /
    std_j, the terms added in constraint order.  0 exactly where every constraint holds."""
    lb, ub, std = (np.asarray(a, dtype=np.float64).ravel() for a in (lb, ub, std))
    c = np.asarray(values, dtype=np.float64).reshape(-1, lb.shape[0])
    total = np.zeros(c.shape[0])
    for j in range(lb.shape[0]):
        total = total + np.maximum(np.maximum(lb[j] - c[:, j], c[:, j] - ub[j]), 0.0) / std[j]
    return total


def observed_violation(space):
    """`violation` of the space's observed rows with std_j = np.std of constraint j's observed column (1 where that is 0) — the
    scale `normalize_y` gives constraint j's GP."""
    cons = space.constraint
    c = np.asarray(space._constraint_values, dtype=np.float64).reshape(len(space), -1)
    std = np.std(c, axis=0) if c.shape[0] else np.ones(c.shape[1])
    return violation(c, cons.lb, cons.ub, np.where(std == 0.0, 1.0, std))


def _fit_models(gp, space, eng, who: str):
    """The target GP, then the constraint GPs, fitted as `fused_acquisition.AcquisitionFunction._fit_gp` fits them (overlapped on
    the device, warnings silenced, theta searches and their RandomState draws included): (the GPs in slot order, their frames)."""
    cons = space.constraint
    overlap = eng.overlapped_fits() if hasattr(eng, "overlapped_fits") else contextlib.nullcontext()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with overlap:
            gp.fit(space.params, space.target)
            cons.fit(space.params, space._constraint_values)
    gps = [gp, *cons.model]
    return gps, [S.read_model(g, space, who) for g in gps]


def constrained_picks(gps, models, space, eng, rng, q: int, n_features: int):
    """q parameter dicts, one per constrained posterior draw over the resident candidates, in groups of at most 16 draws — one
    `sample_paths_constrained` call per group.  Per group and per slot, in slot order 0..C, the draws from `rng`: `spectral_draw`
    with that slot's kernel kind, `standard_normal((S, F))`, `standard_normal((S, N))` scaled by the square root of that slot's
    noise.  The engine call draws nothing; the picked rows are fetched from the device."""
    cons = space.constraint
    y_mean = np.array([m.y_mean for m in models])
    y_std = np.array([m.y_std for m in models])
    picks = []
    for first in range(0, q, MAX_PATHS):
        n = min(MAX_PATHS, q - first)
        draws = []
        for g, m in zip(gps, models):
            omega, phase = spectral_draw(g._kind, n_features, m.d, rng)
            weights = rng.standard_normal((n, n_features))
            eps = rng.standard_normal((n, m.N)) * np.sqrt(m.noise)
            draws.append((omega, phase, weights, eps))
        for g in gps:
            g._ensure_resident()
        out = eng.sample_paths_constrained(draws, cons.lb, cons.ub, y_mean, y_std)
        picks.extend(int(i) for i in out[0])
    rows = np.asarray(eng.get_candidate_rows(np.array(picks, dtype=np.int64), models[0].d), dtype=np.float64)
    return [space.array_to_params(x) for x in rows]


def suggest_constrained_thompson(optimizer, q: int, n_random: int = 10_000, n_features: int = 1024):
    """q parameter dicts to probe side by side, as `suggest_thompson` returns them, for a space WITH a constraint; `optimizer` has
    been `accelerate()`d and its constraint model is a `HipConstraintModel` on the same engine.  In this order:

      1. the argument checks of `suggest_thompson`.
      2. the gate of the suggest functions (below), which here admits the constraint.  The policy is neither consulted nor advanced.
      3. the target GP, then the constraint GPs are fitted on the real data as the policy's own suggest() fits them (overlapped on
         the device), theta searches and their RandomState draws included.
      4. ONE candidate draw of `n_random` points from the optimizer's RandomState, on the device.
      5. ceil(q / 16) `sample_paths_constrained` calls of up to 16 draws.  Each call draws from the optimizer's RandomState, per
         slot in slot order — the objective, constraint 1, ..., constraint C —: `spectral_draw` with that slot's kernel kind (fresh
         features per call and slot), `standard_normal((S, F))` — the feature weights — and `standard_normal((S, N))` scaled by
         sqrt(noise) — the noise draws, noise = that estimator's alpha (+ the WhiteKernel's level for a scaled model).
      6. the picked rows are fetched from the device.
    A draw's pick is the candidate of the largest objective draw among those its constraint draws put inside [lb, ub]; where there
    is none, the candidate of least total violation (include/gpbo.h).  No posterior pass, no local search.  Afterwards `gp.predict`
    and the constraint model answer for the real data as before; slots 0..C hold the fits of step 3.

    ValueError: q not an integer >= 1, n_random < 1, n_features outside [1, 4096], a space without a constraint (use
    `suggest_thompson`).  TargetSpaceEmptyError on an empty space.  NotImplementedError, never a host fallback, for: a GP that is not
    on the engine's slot 0, a space with an input transform, a model in host mode, a device group, a constraint model that is not
    a HipConstraintModel with constraint j's HipGPR in slot j of the same engine on the device path."""
    who = "suggest_constrained_thompson"
    q = S.count(q, 1, None, "q must be an integer >= 1", "q must be >= 1")
    n_random, n_features = int(n_random), int(n_features)
    if n_random < 1:
        raise ValueError("n_random must be >= 1")
    if not 1 <= n_features <= MAX_FEATURES:
        raise ValueError(f"n_features must be in [1, {MAX_FEATURES}]")
    gp, space, eng = S.gate(optimizer, who, "sampled", ("sample_paths_constrained",),
                            "a device group has no path sampler; use a single device", constrained=True)
    if space.constraint is None:
        raise ValueError(f"{who}: the space has no constraint; use suggest_thompson")
    rng = optimizer._random_state

    gps, models = _fit_models(gp, space, eng, who)
    eng.generate_candidates_like(n_random, space.bounds[:, 0], space.bounds[:, 1], rng)
    return constrained_picks(gps, models, space, eng, rng, q, n_features)


class ConstrainedTrustRegion(TrustRegion):
    """`TrustRegion` for a constrained space: `best` counts FEASIBLE targets only, and `best_violation` is the least total
    violation since `origin` (inf before any) — what a batch has to reduce while no feasible point is known."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.best_violation = np.inf

    def observe(self, targets, violations):
        """Take one batch of results into account (an empty batch: nothing happens); violations[i] = the total violation of point i,
        0 = feasible.  The batch IMPROVES iff
          * it holds a feasible point whose target > best + rel_improvement |best| (any feasible point beats best = -inf), or
          * no feasible point has been seen since `origin` (best = -inf), none is in the batch, and the batch's least violation <
            best_violation (1 - rel_improvement).
        Counters, length changes and the restart are `TrustRegion.observe`'s; then best = max(best, the batch's feasible targets)
        and best_violation = min(best_violation, the batch's least violation).  A restart also sets best_violation = inf."""
        targets = np.asarray(targets, dtype=np.float64).ravel()
        violations = np.asarray(violations, dtype=np.float64).ravel()
        if targets.shape != violations.shape:
            raise ValueError("targets and violations must have the same length")
        if targets.size == 0:
            return
        feasible = violations == 0.0
        low = float(violations.min())
        top = float(targets[feasible].max()) if feasible.any() else -np.inf
        if feasible.any():
            improved = self.best == -np.inf or top > self.best + self.rel_improvement * abs(self.best)
        else:
            improved = self.best == -np.inf and low < self.best_violation * (1.0 - self.rel_improvement)
        if improved:
            self.successes, self.failures = self.successes + 1, 0
        else:
            self.successes, self.failures = 0, self.failures + 1
        if self.successes == self.success_tolerance:
            self.length, self.successes = min(2.0 * self.length, self.length_max), 0
        elif self.failures == self.failure_tolerance:
            self.length, self.failures = self.length / 2.0, 0
        self.best = max(self.best, top)
        self.best_violation = min(self.best_violation, low)
        self.seen = (self.seen or 0) + int(targets.size)
        if self.length < self.length_min:
            self.restarts += 1
            self.length = self.length_init
            self.successes = self.failures = 0
            self.best = -np.inf
            self.best_violation = np.inf
            self.origin = self.seen
            self.design_pending = True


def suggest_scbo(optimizer, q: int, state: ConstrainedTrustRegion, n_random: int = 10_000, n_features: int = 1024, perturb=None):
    """q parameter dicts to probe side by side for a space WITH a constraint, by SCBO: `suggest_turbo`'s trust region with the
    picks of `suggest_constrained_thompson`.  `state` is the caller's `ConstrainedTrustRegion(d, q)`, the same object on every call;
    the caller evaluates the points and registers targets and constraint values.  In this order:

      1. the checks below, `suggest_constrained_thompson`'s refusals among them in its order.  The policy is neither consulted nor
         advanced.
      2. the violation of every observed row: sum_j max(lb_j - c_j, c_j - ub_j, 0) / std_j, std_j = np.std of constraint j's observed
         column (1 where that is 0) — the scale `normalize_y` gives constraint j's GP, so the units are the engine's.
      3. `state` catches up: `best_violation` is recomputed over the rows origin..seen with the current stds (they move with the
         data); on the first use seen = len(space) and best = the best feasible target (-inf without one), the counters untouched;
         afterwards `state.observe(space.target[seen:], violation[seen:])`.
      4. if a restart is pending (`state.design_pending`, or nothing has been registered since `state.origin`): `suggest_turbo`'s
         restart design — the two draws of step 6, min(n_random, q) Sobol rows over the WHOLE space generated on the device, the first
         q returned (row i mod the count where n_random < q), `design_pending` cleared.  No fit, no sampling.
      5. the target GP, then the constraint GPs are fitted on ALL the data (theta searches and their RandomState draws included).
         The centre is the best feasible row registered since `state.origin`, else the row of least violation since then; the
         region `state.box(centre, the TARGET GP's length scales, space.bounds)`.
      6. `seed = rng.randint(0, 2**31 - 1)`, then `key = rng.randint(0, 2**63 - 1, dtype=np.int64)` from the optimizer's
         RandomState; `sobol_tables(d, seed)`; `n_random` candidates generated on the device as `suggest_turbo`'s step 5 (`perturb`
         None: min(1, 20 / d)).
      7. ceil(q / 16) `sample_paths_constrained` calls with the draws of `suggest_constrained_thompson`'s step 5 per call — per slot
         in slot order: `spectral_draw`, `standard_normal((S, F))`, `standard_normal((S, N))` scaled by sqrt(noise) — and its pick
         assembly.
    Afterwards `gp.predict` and the constraint model answer for the real data as before.

    ValueError: q not an integer >= 1, n_random outside [1, 2^30], n_features outside [1, 4096], `state` not a
    ConstrainedTrustRegion of the space's dimension and this q, `perturb` not None or a number in (0, 1], a space without a
    constraint (use `suggest_turbo`).  TargetSpaceEmptyError and NotImplementedError as `suggest_constrained_thompson`."""
    who = "suggest_scbo"
    q = S.count(q, 1, None, "q must be an integer >= 1", "q must be >= 1")
    n_random, n_features = int(n_random), int(n_features)
    if not 1 <= n_random <= MAX_CANDIDATES:
        raise ValueError(f"n_random must be in [1, 2^{SOBOL_BITS}]")
    if not 1 <= n_features <= MAX_FEATURES:
        raise ValueError(f"n_features must be in [1, {MAX_FEATURES}]")
    d = int(optimizer._space.bounds.shape[0]) if getattr(optimizer, "_space", None) is not None else None
    if not isinstance(state, ConstrainedTrustRegion) or (d is not None and state.d != d) or state.q != q:
        raise ValueError("state must be a ConstrainedTrustRegion(d, q) of the space's dimension and this q")
    if perturb is not None:
        if isinstance(perturb, bool) or not isinstance(perturb, (int, float, np.integer, np.floating)) or not 0.0 < perturb <= 1.0:
            raise ValueError("perturb must be None or a number in (0, 1]")
    gp, space, eng = S.gate(optimizer, who, "sampled", ("sample_paths_constrained", "generate_candidates_trust_region"),
                            "a device group has no path sampler; use a single device", constrained=True)
    if space.constraint is None:
        raise ValueError(f"{who}: the space has no constraint; use suggest_turbo")
    rng = optimizer._random_state
    probability = min(1.0, 20.0 / d) if perturb is None else float(perturb)

    viol = observed_violation(space)
    target = np.asarray(space.target, dtype=np.float64)
    n = len(space)
    if state.seen is None:
        feasible = viol[state.origin:] == 0.0
        state.seen = n
        state.best = float(np.max(target[state.origin:][feasible])) if feasible.any() else -np.inf
        state.best_violation = float(np.min(viol[state.origin:])) if n > state.origin else np.inf
    else:
        known = viol[state.origin:state.seen]
        state.best_violation = float(np.min(known)) if known.size else np.inf
        state.observe(target[state.seen:], viol[state.seen:])
        state.seen = n

    lo, hi = space.bounds[:, 0], space.bounds[:, 1]
    if state.design_pending or state.origin >= n:
        seed, key = _sobol_seeds(rng)
        sv, shift = sobol_tables(d, seed)
        n_rows = min(n_random, q)
        eng.generate_candidates_trust_region(n_rows, 0.5 * (lo + hi), lo, hi, sv, shift, SOBOL_BITS, 2 ** 32, key)
        rows = np.asarray(eng.get_candidate_rows(np.arange(q, dtype=np.int64) % n_rows, d), dtype=np.float64)
        state.design_pending = False
        return [space.array_to_params(x) for x in rows]

    gps, models = _fit_models(gp, space, eng, who)
    since_v, since_t = viol[state.origin:], target[state.origin:]
    feasible = since_v == 0.0
    row = int(np.argmax(np.where(feasible, since_t, -np.inf))) if feasible.any() else int(np.argmin(since_v))
    centre = np.asarray(space.params[state.origin:][row], dtype=np.float64)
    box = state.box(centre, gp._describe(gp.kernel_).length_scale, space.bounds)
    seed, key = _sobol_seeds(rng)
    sv, shift = sobol_tables(d, seed)
    eng.generate_candidates_trust_region(n_random, centre, box[0], box[1], sv, shift, SOBOL_BITS,
                                         min(2 ** 32, int(probability * 2 ** 32)), key)
    return constrained_picks(gps, models, space, eng, rng, q, n_features)
