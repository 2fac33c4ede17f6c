"""suggest_mes(optimizer) — the next point to probe by max-value entropy search (MES; Wang & Jegelka 2017, "Max-value entropy search
for efficient Bayesian optimization").

Thompson sampling (thompson.py) keeps a posterior draw's maximiser and discards its maximum; MES is the acquisition built on that
value.  A few maxima y*_1 .. y*_S of the posterior are sampled — here the values the engine's `ascend_paths` climbs its draws to —
and each candidate is scored by how much observing it would reduce the entropy of the maximum:

    gamma_s(x) = (y*_s - mu(x)) / sigma(x)
    a(x)       = 1/S sum_s h(gamma_s(x)),      h(g) = g phi(g) / (2 Phi(g)) - log Phi(g)

No incumbent, no xi or kappa.  The values come from ONE posterior pass over the candidates plus S scalars (the engine's
`mes_argbest`, gpbo_mes_argbest; include/gpbo.h has the ranges h is evaluated over and the conventions).
"""
from __future__ import annotations

import numpy as np

from . import _suggest as S
from ._lib import MAX_MES_SAMPLES as MAX_SAMPLES, MAX_PATH_FEATURES as MAX_FEATURES, MAX_PATH_STARTS as MAX_STARTS


def suggest_mes(optimizer, n_samples: int = 16, n_random: int = 10_000, n_features: int = 1024, refine: int = 4, max_iter=None,
                floor_sigmas: float = 5.0, return_info: bool = False):
    """One parameter dict to probe next, as `suggest` returns it; `optimizer` has been `accelerate()`d.

      1. the checks of `suggest_thompson`, with its exception types (below).  The acquisition policy is neither consulted nor advanced.
      2. `gp.fit` on the real data, theta search (and its RandomState draws) included; ONE candidate draw of `n_random` points from
         the optimizer's RandomState, on the device; ONE posterior pass over them, left on the device.
      3. ceil(n_samples / 16) groups of up to 16 posterior draws, one engine call per group: `ascend_paths(n_starts=refine)`, or
         `sample_paths` with `refine=0`.  Each group draws from the optimizer's RandomState in `suggest_thompson`'s order —
         `spectral_draw`, `standard_normal((S, F))`, `standard_normal((S, N))` — so the state ends where
         `suggest_thompson(q=n_samples, refine=refine)` leaves it.  y*_s = the largest finite value draw s was climbed to (without
         one, and with `refine=0`: its maximum among the candidates).
      4. every y*_s is floored at `space.target.max() + floor_sigmas * sqrt(noise) * y_std`, noise = the estimator's alpha (+ the
         WhiteKernel's level for a scaled model) and y_std the targets' normalisation: the floor of the authors' published
         implementation (5 noise standard deviations above the best observation).  It keeps a draw whose climb stopped short from
         putting y* below points already observed; a y* that is not finite takes the floor too.
      5. `mes_argbest(y_star)` over the resident posterior; the picked row is fetched from the device.
    The pick is AMONG THE CANDIDATES: there is no local-search stage.  `return_info=True`: (params, info) with info = {"y_star":
    (n_samples,) the floored maxima, "value": a at the pick, "index": the pick's candidate index}.
    Afterwards `gp.predict` answers for the real data as before; the slot holds the fit of step 2.

    ValueError: n_samples not an integer in [1, 64], n_random < 1, n_features outside [1, 4096], floor_sigmas negative or not finite,
    refine not an integer in [0, 8] (or larger than `n_random`).  TargetSpaceEmptyError on an empty space,
    ConstraintNotSupportedError with a constraint.  NotImplementedError, never a host fallback, for: a GP that is not on the engine's
    slot 0, a space with an input transform (int / categorical parameters), a model in host mode, a device group."""
    n_samples = S.count(n_samples, 1, MAX_SAMPLES, f"n_samples must be an integer in [1, {MAX_SAMPLES}]")
    n_random, n_features = int(n_random), int(n_features)
    if n_random < 1:
        raise ValueError("n_random must be >= 1")
    if not 1 <= n_features <= MAX_FEATURES:
        raise ValueError(f"n_features must be in [1, {MAX_FEATURES}]")
    floor_sigmas = float(floor_sigmas)
    if not np.isfinite(floor_sigmas) or floor_sigmas < 0.0:
        raise ValueError("floor_sigmas must be finite and >= 0")
    gp, space, eng = S.gate(optimizer, "suggest_mes", "sampled", ("sample_paths", "mes_argbest"),
                            "a device group has no path sampler; use a single device")
    refine = S.count(refine, 0, MAX_STARTS, f"refine must be an integer in [0, {MAX_STARTS}]")
    if refine and not hasattr(eng, "ascend_paths"):
        raise NotImplementedError("suggest_mes: the engine has no ascend_paths")
    rng = optimizer._random_state

    model = S.fit_model(gp, space, "suggest_mes")
    eng.generate_candidates_like(n_random, space.bounds[:, 0], space.bounds[:, 1], rng)
    gp._ensure_resident()
    eng.posterior(slot=gp.slot, y_mean=model.y_mean, y_std=model.y_std, fetch=False)
    y_star = np.empty(n_samples)
    for first, n, out in S.draw_groups(gp, space, eng, rng, model, n_samples, n_features, refine, max_iter):
        if refine:
            f = np.where(np.isfinite(out["f"]), out["f"], -np.inf).max(axis=1)
            # (a draw without a finite run keeps its maximum among the candidates)
            y_star[first:first + n] = np.where(np.isfinite(f), f, np.asarray(out["best_val"], dtype=np.float64))
        else:
            y_star[first:first + n] = out[1]
    floor = float(np.max(space.target)) + floor_sigmas * np.sqrt(model.noise) * model.y_std
    y_star = np.where(np.isfinite(y_star) & (y_star > floor), y_star, floor)
    index, value, _seed_idx, _seed_val, _ys = eng.mes_argbest(y_star)
    row = np.asarray(eng.get_candidate_rows(np.array([index], dtype=np.int64), model.d), dtype=np.float64)[0]
    params = space.array_to_params(row)
    if return_info:
        return params, {"y_star": y_star, "value": -float(value), "index": int(index)}
    return params
