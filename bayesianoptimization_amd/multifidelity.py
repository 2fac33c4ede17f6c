"""suggest_multifidelity(optimizer, fidelity) — the next point to probe AND the fidelity to probe it at, by multi-fidelity max-value
entropy search per cost (the GIBBON lower bound; Moss, Leslie & Rayson 2021, "GIBBON: General-purpose Information-Based Bayesian
OptimisatioN").

One of the optimizer's parameters is a fidelity knob (epochs, data fraction, mesh size): cheap below, exact at `target`.  The GP
needs nothing new — the fidelity is an input column.  A candidate z = (x, s) is scored by how much a noisy observation there tells
about the maximum of f(., target), divided by what it costs:

    rho    = corr(y(x, s), f(x, target))                  from the posterior covariance of the pair
    a(z)   = -1/(2S) sum_s log(1 - rho^2 (1 - r2(gamma_s)))      gamma_s = (y*_s - mu(x, target)) / sd(x, target)
    score  = a(z) / (cost0 + cost1 s)

The covariance of the pair, both variances, the score of every candidate and the selection are ONE engine call (`mf_mes_argbest`,
gpmf_mes_argbest; include/gpmf.h has the formulas and the conventions).
"""
from __future__ import annotations

import numpy as np

from . import _suggest as S
from ._lib import MAX_MF_SAMPLES as MAX_SAMPLES, MAX_PATH_FEATURES as MAX_FEATURES


def suggest_multifidelity(optimizer, fidelity, target=None, cost=(1.0, 0.0), n_samples: int = 16, n_random: int = 10_000,
                          n_star: int = 2048, n_features: int = 1024, fidelities=None, floor_sigmas: float = 5.0,
                          return_info: bool = False):
    """One parameter dict to probe next — the fidelity to run at included —, as `suggest` returns it; `optimizer` has been
    `accelerate()`d.  `fidelity`: the name of the parameter that is the fidelity; `target`: the fidelity whose maximum is sought
    (None: the parameter's upper bound); `cost = (cost0, cost1)`: an evaluation at fidelity s costs cost0 + cost1 s.

      1. the checks of `suggest_mes`, with its exception types (below).  The acquisition policy is neither consulted nor advanced.
      2. `gp.fit` on the real data, theta search (and its RandomState draws) included.
      3. `n_star` points at the target fidelity, made on the host from the optimizer's RandomState — one `uniform(lo, hi, n_star)` per
         parameter in column order, the fidelity's column skipped (no draw) and set to `target` — and uploaded.
      4. ceil(n_samples / 16) groups of up to 16 posterior draws over them, one `sample_paths` call per group; each group draws from
         the RandomState in `suggest_thompson`'s order — `spectral_draw`, `standard_normal((S, F))`, `standard_normal((S, N))`.
         y*_s = draw s's maximum among the `n_star` points, floored as `suggest_mes` floors it (`floor_sigmas` noise standard
         deviations above the best observation).  There is NO climb: `ascend_paths` wants box_lo < box_hi in every coordinate and
         cannot hold the fidelity fixed at `target`.
      5. the real candidates, `n_random` of them.  `fidelities=None`: ONE device draw over the whole box (`generate_candidates_like`:
         the RandomState advances as one `uniform(lo, hi, n_random)` per parameter would advance it), the fidelity continuous.
         `fidelities=[...]` (levels inside the fidelity's bounds): on the host, one `uniform(lo, hi, n_random)` per parameter in
         column order, the fidelity's column skipped, then ONE `choice(levels, n_random)` for it; uploaded.
      6. `mf_mes_argbest(y_star, ...)` over them; the picked row is fetched from the device.
    The pick is AMONG THE CANDIDATES: there is no local-search stage.  `return_info=True`: (params, info) with info = {"y_star":
    (n_samples,) the floored maxima, "value": a / cost at the pick, "index": its candidate index, "rho": the pick's correlation with
    its target-fidelity twin, "cost": cost0 + cost1 s at the pick}.
    Afterwards `gp.predict` answers for the real data as before; the slot holds the fit of step 2 and NO resident posterior.

    ValueError: `fidelity` not one of the optimizer's parameters, `target` or a level outside the fidelity's bounds, a cost that is
    not finite or not positive at the fidelity's lower bound (cost0 > 0 and cost1 >= 0 are the engine's terms), n_samples not an
    integer in [1, 64], n_random < 1, n_star < 1, n_features outside [1, 4096], floor_sigmas negative or not finite.
    TargetSpaceEmptyError on an empty space, ConstraintNotSupportedError with a constraint.  NotImplementedError, never a host
    fallback, for: a GP that is not on the engine's slot 0, a space with an input transform (int / categorical parameters), a model
    in host mode, a device group."""
    n_samples = S.count(n_samples, 1, MAX_SAMPLES, f"n_samples must be an integer in [1, {MAX_SAMPLES}]")
    n_random, n_star, n_features = int(n_random), int(n_star), int(n_features)
    if n_random < 1:
        raise ValueError("n_random must be >= 1")
    if n_star < 1:
        raise ValueError("n_star must be >= 1")
    if not 1 <= n_features <= MAX_FEATURES:
        raise ValueError(f"n_features must be in [1, {MAX_FEATURES}]")
    floor_sigmas = float(floor_sigmas)
    if not np.isfinite(floor_sigmas) or floor_sigmas < 0.0:
        raise ValueError("floor_sigmas must be finite and >= 0")
    keys = list(optimizer._space.keys)
    if fidelity not in keys:
        raise ValueError(f"fidelity must be one of the optimizer's parameters {keys}")
    col = keys.index(fidelity)
    lo, hi = (np.asarray(b, dtype=np.float64) for b in (optimizer._space.bounds[:, 0], optimizer._space.bounds[:, 1]))
    target = float(hi[col]) if target is None else float(target)
    if not lo[col] <= target <= hi[col]:
        raise ValueError("target must lie inside the fidelity's bounds")
    cost0, cost1 = (float(c) for c in cost)
    if not (np.isfinite(cost0) and np.isfinite(cost1) and cost0 > 0.0 and cost1 >= 0.0 and cost0 + cost1 * lo[col] > 0.0):
        raise ValueError("cost = (cost0, cost1) must be finite with cost0 > 0, cost1 >= 0 and a positive cost at the fidelity's lower bound")
    if fidelities is not None:
        fidelities = np.atleast_1d(np.asarray(fidelities, dtype=np.float64))
        if fidelities.ndim != 1 or fidelities.size == 0 or not np.all((fidelities >= lo[col]) & (fidelities <= hi[col])):
            raise ValueError("fidelities must be a non-empty sequence of levels inside the fidelity's bounds")
    gp, space, eng = S.gate(optimizer, "suggest_multifidelity", "sampled", ("sample_paths", "mf_mes_argbest"),
                            "a device group has no path sampler; use a single device")
    rng = optimizer._random_state

    model = S.fit_model(gp, space, "suggest_multifidelity")
    others = [t for t in range(model.d) if t != col]

    def host_points(n):
        rows = np.empty((n, model.d))
        for t in others:
            rows[:, t] = rng.uniform(lo[t], hi[t], n)
        return rows

    star = host_points(n_star)
    star[:, col] = target
    eng.set_candidates(star)
    y_star = np.empty(n_samples)
    for first, n, out in S.draw_groups(gp, space, eng, rng, model, n_samples, n_features, 0, None):
        y_star[first:first + n] = out[1]
    floor = float(np.max(space.target)) + floor_sigmas * np.sqrt(model.noise) * model.y_std
    y_star = np.where(np.isfinite(y_star) & (y_star > floor), y_star, floor)

    if fidelities is None:
        eng.generate_candidates_like(n_random, lo, hi, rng)
    else:
        rows = host_points(n_random)
        rows[:, col] = rng.choice(fidelities, n_random)
        eng.set_candidates(rows)
    gp._ensure_resident()
    index, value, _seed_idx, _seed_val, _ys, rho, _mu_t, _sd_t = eng.mf_mes_argbest(
        y_star, col, target, cost0, cost1, y_mean=model.y_mean, y_std=model.y_std, return_parts=True)
    row = np.asarray(eng.get_candidate_rows(np.array([index], dtype=np.int64), model.d), dtype=np.float64)[0]
    params = space.array_to_params(row)
    if return_info:
        return params, {"y_star": y_star, "value": -float(value), "index": int(index), "rho": float(rho[index]),
                        "cost": cost0 + cost1 * float(row[col])}
    return params
