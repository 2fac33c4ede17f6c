"""suggest_jes(optimizer) — the next point to probe by joint entropy search (JES; Hvarfner, Hutter & Nardi 2022, "Joint entropy
search for maximally-informed Bayesian optimization"; Tu et al. 2022; BoTorch's qLowerBoundJointEntropySearch at q = 1).

MES (mes.py) keeps the maxima f*_s its climbed posterior draws reach and discards where they were reached.  JES uses the pair: it
conditions the GP on "the optimum is at x*_s with value f*_s" and scores a candidate by how much observing it lowers the entropy of
that joint,

    a(x) = 1/2 log(var(x) + noise) - 1/S sum_s 1/2 log(vt_s(x) + noise)

with vt_s the variance of f(x) after the conditioning on f(x*_s) = f*_s and the truncation at f*_s.  The values come from ONE
posterior pass over the candidates plus one candidate x sample covariance product on the fp64 matrix cores (the engine's
`jes_argbest`, gpje_jes_argbest; include/gpje.h has the formulas and the conventions).
"""
from __future__ import annotations

import numpy as np

from . import _suggest as S
from ._lib import MAX_JES_SAMPLES as MAX_SAMPLES, MAX_PATH_FEATURES as MAX_FEATURES, MAX_PATH_STARTS as MAX_STARTS


def suggest_jes(optimizer, n_samples: int = 16, n_random: int = 10_000, n_features: int = 1024, refine: int = 4, max_iter=None,
                floor_sigmas: float = 5.0, return_info: bool = False):
    """One parameter dict to probe next, as `suggest` returns it; `optimizer` has been `accelerate()`d.

      1. - 4. are `suggest_mes`'s: the same checks and exception types, `gp.fit`, ONE candidate draw and ONE posterior pass left on
         the device, ceil(n_samples / 16) groups of posterior draws climbed by `ascend_paths(n_starts=refine)` with the same draws
         from the optimizer's RandomState in the same order (the state ends where `suggest_mes` with the same arguments leaves it),
         and the same floor on every f*_s.
      5. x*_s is the `x` of the run that gave f*_s; with `refine=0`, or for a draw without a finite run, the draw's best candidate
         row, fetched from the device.  A floored f*_s keeps its x*_s.
      6. `jes_argbest(x_star, f_star)` over the resident posterior; the picked row is fetched from the device.
    The pick is AMONG THE CANDIDATES.  `return_info=True`: (params, info) with info = {"x_star": (n_samples, d), "f_star":
    (n_samples,) the floored maxima, "value": a at the pick (nats), "index": the pick's candidate index}.

    ValueError, TargetSpaceEmptyError, ConstraintNotSupportedError, NotImplementedError: as `suggest_mes`."""
    n_samples = S.count(n_samples, 1, MAX_SAMPLES, f"n_samples must be an integer in [1, {MAX_SAMPLES}]")
    n_random, n_features = int(n_random), int(n_features)
    if n_random < 1:
        raise ValueError("n_random must be >= 1")
    if not 1 <= n_features <= MAX_FEATURES:
        raise ValueError(f"n_features must be in [1, {MAX_FEATURES}]")
    floor_sigmas = float(floor_sigmas)
    if not np.isfinite(floor_sigmas) or floor_sigmas < 0.0:
        raise ValueError("floor_sigmas must be finite and >= 0")
    gp, space, eng = S.gate(optimizer, "suggest_jes", "sampled", ("sample_paths", "jes_argbest"),
                            "a device group has no path sampler; use a single device")
    refine = S.count(refine, 0, MAX_STARTS, f"refine must be an integer in [0, {MAX_STARTS}]")
    if refine and not hasattr(eng, "ascend_paths"):
        raise NotImplementedError("suggest_jes: the engine has no ascend_paths")
    rng = optimizer._random_state

    model = S.fit_model(gp, space, "suggest_jes")
    eng.generate_candidates_like(n_random, space.bounds[:, 0], space.bounds[:, 1], rng)
    gp._ensure_resident()
    eng.posterior(slot=gp.slot, y_mean=model.y_mean, y_std=model.y_std, fetch=False)
    f_star, x_star = np.empty(n_samples), np.full((n_samples, model.d), np.nan)
    row_of = np.full(n_samples, -1, dtype=np.int64)      # draws whose x* is a candidate row: its index
    for first, n, out in S.draw_groups(gp, space, eng, rng, model, n_samples, n_features, refine, max_iter):
        sl = slice(first, first + n)
        if refine:
            won = out["winner"] >= 0
            f_star[sl] = np.where(won, out["f_best"], np.asarray(out["best_val"], dtype=np.float64))
            x_star[sl] = out["x_best"]
            row_of[sl] = np.where(won, -1, out["best_idx"])
        else:
            row_of[sl], f_star[sl] = out[0], out[1]
    rows = np.flatnonzero(row_of >= 0)
    if rows.size:
        x_star[rows] = np.asarray(eng.get_candidate_rows(row_of[rows], model.d), dtype=np.float64)
    floor = float(np.max(space.target)) + floor_sigmas * np.sqrt(model.noise) * model.y_std
    f_star = np.where(np.isfinite(f_star) & (f_star > floor), f_star, floor)
    index, value, _seed_idx, _seed_val, _ys = eng.jes_argbest(x_star, f_star, y_mean=model.y_mean, y_std=model.y_std)
    row = np.asarray(eng.get_candidate_rows(np.array([index], dtype=np.int64), model.d), dtype=np.float64)[0]
    params = space.array_to_params(row)
    if return_info:
        return params, {"x_star": x_star, "f_star": f_star, "value": -float(value), "index": int(index)}
    return params
