"""suggest_lookahead(optimizer) — the next point to probe by two-step lookahead expected improvement (Ginsbourger & Le Riche 2010;
Wu & Frazier 2019, "Practical two-step look-ahead Bayesian optimization"; BoTorch's qMultiStepLookahead with one fantasy stage).

EI scores a candidate by what its observation is worth now.  Two-step EI adds what the observation is worth for the NEXT choice:

    a(x) = EI(x) + E_y[ max_j EI(a_j | the posterior after observing y at x) ],      j over x itself and J reference points

with the expectation over y by Gauss-Hermite quadrature; per (candidate, node, point) the inner EI is closed-form, so there is no
Monte Carlo.  It is the non-myopic acquisition for near-noiseless objectives, as the knowledge gradient (kg.py) is for noisy ones.
The values come from ONE posterior pass over the candidates plus one candidate x point covariance product on the fp64 matrix cores
(the engine's `ei2_argbest`, gpla_ei2_argbest; include/gpla.h has the formulas and the conventions).
"""
from __future__ import annotations

import numpy as np

from . import _suggest as S
from ._lib import MAX_LA_NODES as MAX_NODES, MAX_LA_POINTS as MAX_POINTS
from .engine import EI


def reference_points(eng, n_points: int, n_candidates: int, y_best: float, return_values: bool = False):
    """(the candidate indices of the reference points, (n_points,); -EI of every candidate or None): the ceil(J / 2) candidates of
    highest EI at xi = 0 against `y_best` (ties to the lowest index) in that order, then the first floor(J / 2) candidate rows not
    among them.  Reads slot 0's resident posterior; draws nothing."""
    n_top = (n_points + 1) // 2
    _i, _v, top, _tv, ys = eng.acq_argbest(EI, 0.0, y_max=y_best, k_seeds=n_top, return_values=return_values)
    top = [int(i) for i in np.asarray(top)[:n_top] if i >= 0]
    taken = set(top)
    rest = []
    for i in range(n_candidates):
        if len(top) + len(rest) >= n_points:
            break
        if i not in taken:
            rest.append(i)
    return np.asarray(top + rest, dtype=np.int64), ys


def suggest_lookahead(optimizer, n_points: int = 32, n_nodes: int = 8, n_random: int = 10_000, return_info: bool = False):
    """One parameter dict to probe next, as `suggest` returns it; `optimizer` has been `accelerate()`d.

      1. the checks below, with `suggest_kg`'s exception types and order.  The acquisition policy is neither consulted nor advanced.
      2. `gp.fit` on the real data, theta search (and its RandomState draws) included; ONE candidate draw of `n_random` points from
         the optimizer's RandomState, on the device; ONE posterior pass over them, left on the device.
      3. the J = `n_points` reference points, with no further random draw: the ceil(J / 2) candidates of highest EI at xi = 0
         against y_best, the largest observed target (ties to the lowest index), then the first floor(J / 2) candidate rows not among
         them; their rows are fetched from the device.
      4. the H = `n_nodes` Gauss-Hermite nodes and weights of a unit normal (`numpy.polynomial.hermite_e.hermegauss`, the weights
         divided by sqrt(2 pi)); `ei2_argbest(points, nodes, weights, y_best)` over the resident posterior; the picked row is fetched
         from the device.
    The pick is AMONG THE CANDIDATES: there is no local-search stage.  `return_info=True`: (params, info) with info =
    {"points_index": (J,) the reference points' candidate indices, "point_means" / "point_vars": (J,) the posterior mean and latent
    variance at them, "value": the two-step EI at the pick, "one_step": plain EI at the pick from the same posterior, "index": the
    pick's candidate index}.
    The optimizer's RandomState ends where the fit and the ONE candidate draw leave it.  Afterwards `gp.predict` answers for the real
    data as before; the slot holds the fit of step 2.

    ValueError: n_points not an integer in [1, 64], n_nodes not an integer in [1, 32], n_random < n_points.  TargetSpaceEmptyError on
    an empty space, ConstraintNotSupportedError with a constraint.  NotImplementedError, never a host fallback, for: a GP that is not
    on the engine's slot 0, a space with an input transform (int / categorical parameters), a model in host mode, a device group."""
    n_points = S.count(n_points, 1, MAX_POINTS, f"n_points must be an integer in [1, {MAX_POINTS}]")
    n_nodes = S.count(n_nodes, 1, MAX_NODES, f"n_nodes must be an integer in [1, {MAX_NODES}]")
    n_random = int(n_random)
    if n_random < n_points:
        raise ValueError("n_random must be >= n_points")
    gp, space, eng = S.gate(optimizer, "suggest_lookahead", "scored", ("ei2_argbest",),
                            "a device group has no two-step lookahead EI; use a single device")
    rng = optimizer._random_state

    model = S.fit_model(gp, space, "suggest_lookahead")
    eng.generate_candidates_like(n_random, space.bounds[:, 0], space.bounds[:, 1], rng)
    gp._ensure_resident()
    eng.posterior(slot=gp.slot, y_mean=model.y_mean, y_std=model.y_std, fetch=False)
    y_best = float(np.max(space.target))
    points_index, neg_ei = reference_points(eng, n_points, n_random, y_best, return_values=return_info)
    points = np.asarray(eng.get_candidate_rows(points_index, model.d), dtype=np.float64)
    nodes, weights = np.polynomial.hermite_e.hermegauss(n_nodes)
    index, value, _seed_idx, _seed_val, _ys, point_means, point_vars = eng.ei2_argbest(
        points, nodes, weights / np.sqrt(2.0 * np.pi), y_best, y_mean=model.y_mean, y_std=model.y_std, return_point_moments=True)
    row = np.asarray(eng.get_candidate_rows(np.array([index], dtype=np.int64), model.d), dtype=np.float64)[0]
    params = space.array_to_params(row)
    if return_info:
        return params, {"points_index": points_index, "point_means": np.asarray(point_means, dtype=np.float64),
                        "point_vars": np.asarray(point_vars, dtype=np.float64), "value": -float(value),
                        "one_step": -float(neg_ei[index]), "index": int(index)}
    return params
