"""suggest_ivr(optimizer) — the next point to probe by integrated posterior variance reduction (Cohn 1996, "Neural network
exploration using optimal experiment design": ALC; Sacks, Welch, Mitchell & Wynn 1989: IMSE-optimal design; BoTorch's
qNegIntegratedPosteriorVariance at q = 1).

UCB / EI / POI score a candidate by its own posterior value, Thompson sampling, MES and qNEI by posterior draws, KG by the maximum
of the posterior mean.  This one scores a candidate by what observing it teaches about the surrogate EVERYWHERE: how much one noisy
observation at x lowers the latent posterior variance, averaged over J integration points a_1 .. a_J spread over the box,

    IVR(x) = sum_j omega_j cov(x, a_j)^2 / (var(x) + noise)

— the acquisition for building an accurate surrogate before or beside optimising: active learning, calibration runs, the
exploration phase of a noisy campaign.  The values come from ONE posterior pass over the candidates plus one candidate x point
covariance product on the fp64 matrix cores at 2 N J flops per candidate (the engine's `ivr_argbest`, gpiv_ivr_argbest;
include/gpiv.h has the formulas and the conventions).
"""
from __future__ import annotations

import numpy as np

from . import _suggest as S
from ._lib import MAX_IVR_POINTS as MAX_POINTS


def suggest_ivr(optimizer, n_points: int = 1024, n_random: int = 10_000, weights=None, return_info: bool = False):
    """One parameter dict to probe next, as `suggest` returns it; `optimizer` has been `accelerate()`d.

      1. the checks below, with `suggest_kg`'s exception types and order.  The acquisition policy is neither consulted nor advanced.
      2. `gp.fit` on the real data, theta search (and its RandomState draws) included; ONE candidate draw of `n_random` points from
         the optimizer's RandomState, on the device; ONE posterior pass over them, left on the device.
      3. the J = `n_points` integration points, with no further random draw: the first J candidate rows — the rows are i.i.d.
         uniform over the box, so they are a Monte-Carlo sample of it; their rows are fetched from the device.  `weights` (J,) or
         None = 1 / J each.
      4. `ivr_argbest(points, weights)` over the resident posterior; the picked row is fetched from the device.
    The pick is AMONG THE CANDIDATES: there is no local-search stage.  `return_info=True`: (params, info) with info =
    {"points_index": (J,) the integration points' candidate indices, "value": IVR at the pick, "index": the pick's candidate index}.
    The optimizer's RandomState ends where the fit and the ONE candidate draw leave it, as after `suggest_kg`.  Afterwards
    `gp.predict` answers for the real data as before; the slot holds the fit of step 2.

    ValueError: n_points not an integer in [1, 4096], n_random < n_points.  TargetSpaceEmptyError on an empty space,
    ConstraintNotSupportedError with a constraint.  NotImplementedError, never a host fallback, for: a GP that is not on the engine's
    slot 0, a space with an input transform (int / categorical parameters), a model in host mode, a device group."""
    n_points = S.count(n_points, 1, MAX_POINTS, f"n_points must be an integer in [1, {MAX_POINTS}]")
    n_random = int(n_random)
    if n_random < n_points:
        raise ValueError("n_random must be >= n_points")
    gp, space, eng = S.gate(optimizer, "suggest_ivr", "scored", ("ivr_argbest",),
                            "a device group has no integrated variance reduction; use a single device")
    rng = optimizer._random_state

    model = S.fit_model(gp, space, "suggest_ivr")
    eng.generate_candidates_like(n_random, space.bounds[:, 0], space.bounds[:, 1], rng)
    gp._ensure_resident()
    eng.posterior(slot=gp.slot, y_mean=model.y_mean, y_std=model.y_std, fetch=False)
    points_index = np.arange(n_points, dtype=np.int64)
    points = np.asarray(eng.get_candidate_rows(points_index, model.d), dtype=np.float64)
    index, value, _seed_idx, _seed_val, _ys = eng.ivr_argbest(points, weights, y_mean=model.y_mean, y_std=model.y_std)
    row = np.asarray(eng.get_candidate_rows(np.array([index], dtype=np.int64), model.d), dtype=np.float64)[0]
    params = space.array_to_params(row)
    if return_info:
        return params, {"points_index": points_index, "value": -float(value), "index": int(index)}
    return params
