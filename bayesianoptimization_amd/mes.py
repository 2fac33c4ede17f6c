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

import warnings

import numpy as np

from . import fused_acquisition as A
from ._lib import MAX_MES_SAMPLES as MAX_SAMPLES, MAX_PATH_FEATURES as MAX_FEATURES, MAX_PATH_STARTS as MAX_STARTS, MAX_PATHS
from .engine import GroupEngine
from .gpr import HipGPR
from .thompson import spectral_draw


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
    if isinstance(n_samples, bool) or not isinstance(n_samples, (int, np.integer)) or not 1 <= int(n_samples) <= MAX_SAMPLES:
        raise ValueError(f"n_samples must be an integer in [1, {MAX_SAMPLES}]")
    n_samples = int(n_samples)
    n_random, n_features = int(n_random), int(n_features)
    if n_random < 1:
        raise ValueError("n_random must be >= 1")
    if not 1 <= n_features <= MAX_FEATURES:
        raise ValueError(f"n_features must be in [1, {MAX_FEATURES}]")
    floor_sigmas = float(floor_sigmas)
    if not np.isfinite(floor_sigmas) or floor_sigmas < 0.0:
        raise ValueError("floor_sigmas must be finite and >= 0")
    gp = optimizer._gp
    space = optimizer._space
    if not isinstance(gp, HipGPR) or gp.slot != 0:
        raise NotImplementedError("suggest_mes: the optimizer's GP is not on the engine (call accelerate(optimizer) first)")
    if len(space) == 0:
        raise A.TargetSpaceEmptyError("Cannot suggest a point without previous samples. Use "
                                      " target_space.random_sample() to generate a point and "
                                      " target_space.probe(*) to evaluate it.")
    if space.constraint is not None:
        raise A.ConstraintNotSupportedError("Received constraints, but suggest_mes does not support constrained optimization.")
    if gp.transform is not None:
        raise NotImplementedError("suggest_mes: the space has an input transform (int / categorical parameters); "
                                  "only all-float spaces are sampled")
    eng = gp._engine()
    if isinstance(eng, GroupEngine):
        raise NotImplementedError("suggest_mes: a device group has no path sampler; use a single device")
    if not hasattr(eng, "sample_paths") or not hasattr(eng, "mes_argbest"):
        raise NotImplementedError("suggest_mes: the engine has no sample_paths / mes_argbest")
    from sklearn.base import clone

    reason = None if gp.kernel is None else gp._unsupported_reason(clone(gp.kernel), space.target, space.params)
    if reason is not None:
        raise NotImplementedError(f"suggest_mes: the model runs on the host ({reason}); only models on the device path are sampled")
    if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)) or not 0 <= int(refine) <= MAX_STARTS:
        raise ValueError(f"refine must be an integer in [0, {MAX_STARTS}]")
    refine = int(refine)
    if refine and not hasattr(eng, "ascend_paths"):
        raise NotImplementedError("suggest_mes: the engine has no ascend_paths")
    rng = optimizer._random_state

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp.fit(space.params, space.target)
    if gp._host_mode:      # (unreachable after the check above; a host model must not get this far silently)
        raise NotImplementedError("suggest_mes: the model was fitted on the host")
    d = int(space.bounds.shape[0])
    N = int(gp.X_train_.shape[0])
    y_mean, y_std = float(gp._y_train_mean), float(gp._y_train_std)
    scale = gp.__dict__.get("_scale")
    noise = float(gp.alpha) + (0.0 if scale is None else float(scale[1]))
    eng.generate_candidates_like(n_random, space.bounds[:, 0], space.bounds[:, 1], rng)
    gp._ensure_resident()
    eng.posterior(slot=gp.slot, y_mean=y_mean, y_std=y_std, fetch=False)
    y_star = np.empty(n_samples)
    for first in range(0, n_samples, MAX_PATHS):
        S = min(MAX_PATHS, n_samples - first)
        omega, phase = spectral_draw(gp._kind, n_features, d, rng)
        weights = rng.standard_normal((S, n_features))
        eps = rng.standard_normal((S, N)) * np.sqrt(noise)
        gp._ensure_resident()
        if refine:
            out = eng.ascend_paths(omega, phase, weights, eps, space.bounds[:, 0], space.bounds[:, 1], n_starts=refine,
                                   max_iter=-1 if max_iter is None else int(max_iter), slot=gp.slot, y_mean=y_mean, y_std=y_std)
            f = np.where(np.isfinite(out["f"]), out["f"], -np.inf).max(axis=1)
            # (a draw without a finite run keeps its maximum among the candidates)
            y_star[first:first + S] = np.where(np.isfinite(f), f, np.asarray(out["best_val"], dtype=np.float64))
        else:
            _best, val, _values = eng.sample_paths(omega, phase, weights, eps, slot=gp.slot, y_mean=y_mean, y_std=y_std)
            y_star[first:first + S] = val
    floor = float(np.max(space.target)) + floor_sigmas * np.sqrt(noise) * y_std
    y_star = np.where(np.isfinite(y_star) & (y_star > floor), y_star, floor)
    index, value, _seed_idx, _seed_val, _ys = eng.mes_argbest(y_star)
    row = np.asarray(eng.get_candidate_rows(np.array([index], dtype=np.int64), d), dtype=np.float64)[0]
    params = space.array_to_params(row)
    if return_info:
        return params, {"y_star": y_star, "value": -float(value), "index": int(index)}
    return params
