"""suggest_constrained_qnei(optimizer, q) — q points to probe in parallel by batch noisy expected improvement UNDER CONSTRAINTS
(Letham, Karrer, Ottoni & Bakshy 2019, "Constrained Bayesian optimization with noisy experiments").

`suggest_qnei` (qnei.py) scores a batch jointly over T posterior draws of the objective, each with an incumbent of its own.  With
constraints that are themselves noisy GPs, feasibility is uncertain too.  Here every joint draw t carries a draw of the objective AND
of each constraint; a point counts for draw t only where the draw's constraints hold,

    g_t(x) = f_t(x)  where every constraint draw puts x inside [lb, ub],   -inf elsewhere,
    a(x)   = 1/T sum_t max(g_t(x) - m_t, 0),       m_t = max(floor, max_i g_t(x_i) over the observed and pending points),

so a draw in which no observed point is feasible starts from `floor` (the paper's M) and rewards ANY feasible point, and a draw
whose constraints call x infeasible contributes nothing.  The batch is built greedily as `suggest_qnei` builds it — after a pick
every draw's incumbent absorbs g_t(pick) — in ONE engine call (`cnei_greedy`, gpbo_cnei_greedy; include/gpbo.h has the rule).
Constrained Thompson picks (scbo.py) are independent of each other; these are scored jointly.
"""
from __future__ import annotations

import numpy as np

from . import _suggest as S
from ._lib import MAX_CNEI_BASE as MAX_BASE
from .scbo import _fit_models


def default_floor(target) -> float:
    """The incumbent of a draw without a feasible point when the caller names none: target.min() - ptp(target), or target.min() - 1
    where the range is 0 — below every measurement by the measurements' own range, so that any feasible point is an improvement
    and a better one a larger improvement."""
    target = np.asarray(target, dtype=np.float64)
    lo, span = float(target.min()), float(np.ptp(target))
    return lo - (span if span > 0.0 else 1.0)


def suggest_constrained_qnei(optimizer, q: int, n_random: int = 10_000, n_draws: int = 64, n_features: int = 1024, pending=None,
                             floor=None, return_info: bool = False):
    """q parameter dicts to probe side by side, as `suggest_qnei` returns them, for a space WITH a constraint; `optimizer` has been
    `accelerate()`d and its constraint model is a `HipConstraintModel` on the same engine.  In this order:

      1. `suggest_qnei`'s argument checks, with its exception types.  The acquisition policy is neither consulted nor advanced.
      2. the gate of the suggest functions, which here admits the constraint; then ValueError on a space without one.
      3. the target GP, then the constraint GPs are fitted on the real data (`scbo._fit_models`: overlapped on the device), theta
         searches and their RandomState draws included.
      4. ONE candidate draw of `n_random` points from the optimizer's RandomState, on the device.
      5. G x S draws (`draw_layout(n_draws)`: T = G * S >= n_draws).  Per group, and within a group per slot in slot order — the
         objective, constraint 1, ..., constraint C —, from the optimizer's RandomState: `spectral_draw` with that slot's kernel
         kind, `standard_normal((S, F))`, `standard_normal((S, N))` scaled by sqrt(that slot's noise) — `constrained_picks`' draws.
      6. ONE `cnei_greedy` call with `base` = the observed params followed by `pending` (a list of parameter dicts or an array
         (P, d)) and `y_floor` = `floor`; `floor=None` is `default_floor(space.target)`: target.min() - ptp(target), or
         target.min() - 1 where the range is 0.
      7. the picked rows are fetched from the device.
    The zero-gain tail of `suggest_qnei` applies: when no draw finds a feasible candidate above its incumbent, every gain is 0 and
    the lowest unpicked indices are handed out — there is no least-violation fallback; info["gain"] and info["feasible"] say so.
    `return_info=True`: (picks, info) with info = {"gain" (q,), "index" (q,), "feasible" (q,): the share of draws that call each pick
    feasible, "baseline" (T,): the incumbents before the first pick, "n_draws": T}.

    ValueError: the count and range errors of `suggest_qnei` (q, n_random, n_draws, n_features), more than 16384 observed + pending
    points, pending of another shape or not finite, a floor that is not finite, a space without a constraint (use suggest_qnei).
    TargetSpaceEmptyError on an empty space.  NotImplementedError, never a host fallback: `suggest_constrained_thompson`'s cases."""
    who = "suggest_constrained_qnei"
    q, n_random, n_draws, n_features = S.greedy_counts(q, n_random, n_draws, n_features)
    if floor is not None and not np.isfinite(floor):
        raise ValueError("floor must be finite")
    gp, space, eng = S.gate(optimizer, who, "batched", ("cnei_greedy",), "a device group has no path sampler; use a single device",
                            constrained=True)
    if space.constraint is None:
        raise ValueError(f"{who}: the space has no constraint; use suggest_qnei")
    pending = S.pending_rows(pending, space, int(space.bounds.shape[0]))
    base = np.asarray(space.params, dtype=np.float64)
    if pending is not None:
        base = np.concatenate([base, pending])
    if base.shape[0] > MAX_BASE:
        raise ValueError(f"the observed and pending points must number at most {MAX_BASE}")
    rng = optimizer._random_state

    gps, models = _fit_models(gp, space, eng, who)
    eng.generate_candidates_like(n_random, space.bounds[:, 0], space.bounds[:, 1], rng)
    G, n_paths = S.draw_layout(n_draws)
    draws = S.group_inputs(list(gps), rng, list(models), G, n_paths, n_features)
    for g in gps:
        g._ensure_resident()
    cons = space.constraint
    out = eng.cnei_greedy(draws, q, cons.lb, cons.ub, default_floor(space.target) if floor is None else float(floor),
                          base=np.ascontiguousarray(base), y_mean=[m.y_mean for m in models], y_std=[m.y_std for m in models])
    index, picks = S.picked_params(eng, out["index"], models[0].d, space.array_to_params)
    if return_info:
        return picks, {"gain": np.asarray(out["gain"], dtype=np.float64), "index": index,
                       "feasible": np.asarray(out["feasible"], dtype=np.float64),
                       "baseline": np.asarray(out["baseline"], dtype=np.float64), "n_draws": G * n_paths}
    return picks
