"""suggest_levelset(optimizer, level) — the next point to probe to learn WHERE the target crosses `level`: stepwise uncertainty
reduction (SUR) for the excursion set {x : f(x) > level} (Bect, Ginsbourger, Li, Picheny & Vazquez 2012, "Sequential design of
computer experiments for the estimation of a probability of failure"; closed form by Chevalier, Bect, Ginsbourger, Vazquez, Picheny
& Richet 2014, "Fast parallel kriging-based stepwise uncertainty reduction with application to the identification of an excursion
set").

UCB / EI / POI and the entropy searches ask about the optimum, `suggest_ivr` about the surrogate everywhere.  This one asks about a
contour: the boundary of a feasible region, a failure domain, a level curve to map.  Over J integration points a_j spread over the
box the current classification uncertainty is

    U = sum_j omega_j p_j (1 - p_j),        p_j = P(f(a_j) > level)

and a candidate x is scored by the expected drop of U after one noisy observation at x — large where the observation is correlated
with points whose side of the level is still undecided.  The values come from ONE posterior pass over the candidates plus the
candidate x point covariance product of `suggest_ivr` with a bivariate normal probability per (candidate, point) behind it, in
registers (the engine's `sur_argbest`, gpls_sur_argbest; include/gpls.h has the formulas and the conventions).  U itself comes back
with the pick: it is the quantity to stop on.
"""
from __future__ import annotations

import numpy as np

from . import _suggest as S
from ._lib import MAX_LS_POINTS as MAX_POINTS


def suggest_levelset(optimizer, level: float, n_points: int = 1024, n_random: int = 10_000, points=None, weights=None,
                     return_info: bool = False):
    """One parameter dict to probe next, as `suggest` returns it; `optimizer` has been `accelerate()`d.  `level`: raw target units.

      1. the checks below, with `suggest_ivr`'s exception types and order.  The acquisition policy is neither consulted nor advanced.
      2. `gp.fit` on the real data, theta search (and its RandomState draws) included; ONE candidate draw of `n_random` points from
         the optimizer's RandomState, on the device; ONE posterior pass over them, left on the device.
      3. the J integration points, with no further random draw: `points` (J, d) of the caller's, parameter space, in the order of
         the space's keys — or, `points` None, the first J = `n_points` candidate rows, which are i.i.d. uniform over the box and so a
         Monte-Carlo sample of it.  `weights` (J,) or None = 1 / J each.
      4. `sur_argbest(points, level, weights)` over the resident posterior; the picked row is fetched from the device.
    The pick is AMONG THE CANDIDATES: there is no local-search stage.  `return_info=True`: (params, info) with info = {"points": (J, d)
    the integration points, "p": (J,) their excursion probabilities P(f(a_j) > level), "uncertainty": sum_j omega_j p_j (1 - p_j)
    BEFORE the observation, "value": its expected reduction at the pick, "index": the pick's candidate index}.  The optimizer's
    RandomState ends where the fit and the ONE candidate draw leave it, as after `suggest_ivr`.

    ValueError: level not a finite number; n_points not an integer in [1, 4096] or points not (J, d) with J in that range;
    n_random < n_points (points None).  TargetSpaceEmptyError on an empty space, ConstraintNotSupportedError with a constraint.
    NotImplementedError, never a host fallback, for: a GP that is not on the engine's slot 0, a space with an input transform (int /
    categorical parameters), a model in host mode, a device group."""
    level = float(level)
    if not np.isfinite(level):
        raise ValueError("level must be a finite number")
    n_random = int(n_random)
    if points is None:
        n_points = S.count(n_points, 1, MAX_POINTS, f"n_points must be an integer in [1, {MAX_POINTS}]")
        if n_random < n_points:
            raise ValueError("n_random must be >= n_points")
    else:
        points = np.ascontiguousarray(np.asarray(points, dtype=np.float64))
        if points.ndim != 2 or not 1 <= points.shape[0] <= MAX_POINTS:
            raise ValueError(f"points must be (J, d) with J in [1, {MAX_POINTS}]")
    gp, space, eng = S.gate(optimizer, "suggest_levelset", "scored", ("sur_argbest",),
                            "a device group has no level-set acquisition; use a single device")
    rng = optimizer._random_state

    model = S.fit_model(gp, space, "suggest_levelset")
    eng.generate_candidates_like(n_random, space.bounds[:, 0], space.bounds[:, 1], rng)
    gp._ensure_resident()
    eng.posterior(slot=gp.slot, y_mean=model.y_mean, y_std=model.y_std, fetch=False)
    if points is None:
        points = np.asarray(eng.get_candidate_rows(np.arange(n_points, dtype=np.int64), model.d), dtype=np.float64)
    index, value, _seed_idx, _seed_val, _ys, p, uncertainty = eng.sur_argbest(points, level, weights, y_mean=model.y_mean,
                                                                              y_std=model.y_std, return_points=True)
    row = np.asarray(eng.get_candidate_rows(np.array([index], dtype=np.int64), model.d), dtype=np.float64)[0]
    params = space.array_to_params(row)
    if return_info:
        return params, {"points": points, "p": p, "uncertainty": float(uncertainty), "value": -float(value), "index": int(index)}
    return params
