"""suggest_kg(optimizer) — the next point to probe by the knowledge gradient (KG; Frazier, Powell & Dayanik 2009, "The
knowledge-gradient policy for correlated normal beliefs"; Scott, Frazier & Powell 2011 for continuous parameters).

UCB / EI / POI score a candidate by its own posterior value, Thompson sampling and MES (thompson.py, mes.py) by posterior draws.
KG looks one step AHEAD: it scores a candidate by how much observing it would raise the maximum of the posterior MEAN — the point
one would recommend in the end.  That is the acquisition for noisy objectives, where EI's incumbent is itself a noisy number.  In
its discrete form the maximum runs over the candidate itself and J reference points a_1 .. a_J:

    KG(x) = E_Z[ max_j (a_j + b_j(x) Z) ] - max_j a_j,      Z ~ N(0, 1)
    (a_0, b_0) = (mu(x), var(x) / sd_obs(x)),    (a_j, b_j) = (mu(a_j), cov(x, a_j) / sd_obs(x))

the upper envelope of J + 1 lines, evaluated exactly.  The values come from ONE posterior pass over the candidates plus one
candidate x point covariance pass at O(N d + N J) per candidate (the engine's `kg_argbest`, gpbo_kg_argbest; include/gpbo.h has
the formulas and the conventions).
"""
from __future__ import annotations

import numpy as np

from . import _suggest as S
from ._lib import MAX_KG_POINTS as MAX_POINTS
from .engine import UCB


def reference_points(eng, n_points: int, n_candidates: int) -> np.ndarray:
    """The candidate indices of the reference points, (n_points,): the ceil(J / 2) candidates of highest posterior mean (ties to
    the lowest index) in that order, then the first floor(J / 2) candidate rows not among them — the rows are i.i.d. uniform, so
    the first rows are a random subset.  Reads slot 0's resident posterior (`acq_argbest` with UCB at kappa = 0); draws nothing."""
    n_top = (n_points + 1) // 2
    _i, _v, top, _tv, _ys = eng.acq_argbest(UCB, 0.0, k_seeds=n_top)
    top = [int(i) for i in np.asarray(top)[:n_top] if i >= 0]
    taken = set(top)
    rest = []
    for i in range(n_candidates):
        if len(top) + len(rest) >= n_points:
            break
        if i not in taken:
            rest.append(i)
    return np.asarray(top + rest, dtype=np.int64)


def suggest_kg(optimizer, n_points: int = 32, n_random: int = 10_000, return_info: bool = False):
    """One parameter dict to probe next, as `suggest` returns it; `optimizer` has been `accelerate()`d.

      1. the checks below, with `suggest_mes`' exception types and order.  The acquisition policy is neither consulted nor advanced.
      2. `gp.fit` on the real data, theta search (and its RandomState draws) included; ONE candidate draw of `n_random` points from
         the optimizer's RandomState, on the device; ONE posterior pass over them, left on the device.
      3. the J = `n_points` reference points, with no further random draw: the ceil(J / 2) candidates of highest posterior mean
         (ties to the lowest index), then the first floor(J / 2) candidate rows not among them; their rows are fetched from the device.
      4. `kg_argbest(points)` over the resident posterior; the picked row is fetched from the device.
    The pick is AMONG THE CANDIDATES: there is no local-search stage.  `return_info=True`: (params, info) with info =
    {"points_index": (J,) the reference points' candidate indices, "point_means": (J,) the posterior mean at them, "value": KG at
    the pick, "index": the pick's candidate index}.
    The optimizer's RandomState ends where the fit and the ONE candidate draw leave it: neither the reference points nor the
    engine call draw from it.  Afterwards `gp.predict` answers for the real data as before; the slot holds the fit of step 2.

    ValueError: n_points not an integer in [1, 64], n_random < n_points.  TargetSpaceEmptyError on an empty space,
    ConstraintNotSupportedError with a constraint.  NotImplementedError, never a host fallback, for: a GP that is not on the engine's
    slot 0, a space with an input transform (int / categorical parameters), a model in host mode, a device group."""
    n_points = S.count(n_points, 1, MAX_POINTS, f"n_points must be an integer in [1, {MAX_POINTS}]")
    n_random = int(n_random)
    if n_random < n_points:
        raise ValueError("n_random must be >= n_points")
    gp, space, eng = S.gate(optimizer, "suggest_kg", "scored", ("kg_argbest",),
                            "a device group has no knowledge gradient; use a single device")
    rng = optimizer._random_state

    model = S.fit_model(gp, space, "suggest_kg")
    eng.generate_candidates_like(n_random, space.bounds[:, 0], space.bounds[:, 1], rng)
    gp._ensure_resident()
    eng.posterior(slot=gp.slot, y_mean=model.y_mean, y_std=model.y_std, fetch=False)
    points_index = reference_points(eng, n_points, n_random)
    points = np.asarray(eng.get_candidate_rows(points_index, model.d), dtype=np.float64)
    index, value, _seed_idx, _seed_val, _ys, point_means = eng.kg_argbest(points, y_mean=model.y_mean, y_std=model.y_std,
                                                                          return_point_means=True)
    row = np.asarray(eng.get_candidate_rows(np.array([index], dtype=np.int64), model.d), dtype=np.float64)[0]
    params = space.array_to_params(row)
    if return_info:
        return params, {"points_index": points_index, "point_means": np.asarray(point_means, dtype=np.float64),
                        "value": -float(value), "index": int(index)}
    return params
