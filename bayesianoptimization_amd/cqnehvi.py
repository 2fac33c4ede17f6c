"""suggest_constrained_qnehvi(pareto, q) — q points to probe in parallel for TWO noisy objectives UNDER NOISY CONSTRAINTS, by batch
noisy expected hypervolume improvement in its constrained form (Daulton, Balandat & Bakshy 2021, "Parallel Bayesian optimization
of multiple noisy objectives with expected hypervolume improvement").

`suggest_qnehvi` (qnehvi.py) gives every joint draw of the two objectives a Pareto front of its own.  With constraints that are
themselves noisy GPs, feasibility is uncertain too.  Here every joint draw t carries a draw of both objectives AND of each
constraint; a point counts for draw t only where the draw's constraints hold,

    g0_t(x) = f0_t(x)  where every constraint draw puts x inside [lb, ub],   -inf elsewhere,
    a(x)    = 1/T sum_t HVI((g0_t(x), f1_t(x)) | P_t),      P_t the front of the draw's FEASIBLE observed and pending points,

so a draw's front holds only what that draw calls feasible — the draws decide, not the noisy readings —, and a draw whose
constraints call x infeasible contributes nothing.  The batch is built greedily as `suggest_qnehvi` builds it, in ONE engine call
(`cnehvi_greedy`, gpmo_cnhvi_greedy; include/gpmo.h has the rule).  m = 2 only.
"""
from __future__ import annotations

import contextlib
import warnings

import numpy as np

from . import _suggest as S
from ._lib import MAX_QNEHVI_BASE as MAX_BASE


def suggest_constrained_qnehvi(pareto, q: int, n_random: int = 10_000, n_draws: int = 64, n_features: int = 1024, pending=None,
                               return_info: bool = False):
    """q parameter dicts to probe side by side for the two objectives of `pareto`, a `ParetoOptimizer` WITH `constraints`.  In this
    order:

      1. `suggest_qnehvi`'s argument checks (ValueError).
      2. the refusals: NotImplementedError for `n_objectives == 3`; ValueError for an optimizer without constraints (use
         suggest_qnehvi); then `suggest_qnehvi`'s — TargetSpaceEmptyError on an empty store, NotImplementedError (never a host
         fallback) for a device group and for an objective or a constraint whose model would run on the host.  ValueError when the
         observed and the pending points together exceed 16384.
      3. the two objectives' fits, then the C constraints', on the observations in slot order, overlapped on the device where the
         engine can, warnings silenced; each fit's theta search draws from the RandomState, in slot order.
      4. ONE candidate draw of `n_random` points from the RandomState, on the device, as `suggest` draws it.
      5. G x S draws (`draw_layout(n_draws)`: T = G * S >= n_draws).  Per group, and within a group per slot in slot order — objective
         0, objective 1, constraint 0, ..., constraint C - 1 —, from the RandomState: `spectral_draw` with that slot's kernel kind,
         `standard_normal((S, F))`, `standard_normal((S, N))` scaled by sqrt(that slot's noise) — `suggest_constrained_qnei`'s
         draws (`group_inputs` over the 2 + C models).
      6. ONE `cnehvi_greedy` call with `base` = ALL observed params followed by `pending` (a list of parameter dicts or an array
         (P, d)): the draws decide which of them are feasible.
      7. the picked rows are fetched from the device.
    The zero-gain tail of `suggest_qnehvi` applies: when no draw gains anything, every gain is 0 and the lowest unpicked indices are
    handed out — there is no least-violation fallback; info["gain"] and info["feasible"] say so.
    `return_info=True`: (picks, info) with info = {"gain" (q,), "index" (q,), "feasible" (q,): the share of draws that call each pick
    feasible, "front_size_before" / "front_size_after": the largest front of any draw before the first pick / after the last,
    "n_draws": T}.

    ValueError: as `suggest_qnehvi`, and an optimizer without constraints.  NotImplementedError also when a draw's front outgrows
    128 points."""
    who = "suggest_constrained_qnehvi"
    q, n_random, n_draws, n_features = S.greedy_counts(q, n_random, n_draws, n_features)
    d = int(pareto.bounds.shape[0])
    pending = S.pending_rows(pending, pareto, d)
    if pareto.n_objectives != 2:
        raise NotImplementedError(f"{who}: {pareto.n_objectives} objectives; a draw's front is a staircase for two objectives "
                                  "only (gpmo_cnhvi_greedy serves m = 2 and approximates nothing)")
    if getattr(pareto, "constraints", None) is None:
        raise ValueError(f"{who}: the optimizer has no constraints; use suggest_qnehvi")
    eng = S.pareto_gate(pareto, who, "constrained batch noisy expected hypervolume improvement")
    host = pareto._constraint_host_reason()
    if host is not None:
        raise NotImplementedError(f"{who}: constraint {host[0]}'s model runs on the host ({host[1]}); only models on the device path "
                                  "are served")
    if not hasattr(eng, "cnehvi_greedy"):
        raise NotImplementedError(f"{who}: the engine has no cnehvi_greedy")
    base = pareto.params if pending is None else np.concatenate([pareto.params, pending])
    if base.shape[0] > MAX_BASE:
        raise ValueError(f"the observed and the pending points together must not exceed {MAX_BASE}")
    rng = pareto._random_state

    gps = list(pareto._gps) + list(pareto._cgps)
    columns = [pareto.targets[:, j] for j in range(2)] + [pareto.constraint_values[:, j] for j in range(len(pareto._cgps))]
    overlap = eng.overlapped_fits() if hasattr(eng, "overlapped_fits") else contextlib.nullcontext()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with overlap:
            for gp, y in zip(gps, columns):
                gp.fit(pareto.params, y)
    models = [S.read_model(gp, pareto, who) for gp in gps]
    eng.generate_candidates_like(n_random, pareto.bounds[:, 0], pareto.bounds[:, 1], rng)
    G, n_paths = S.draw_layout(n_draws)
    draws = S.group_inputs(gps, rng, models, G, n_paths, n_features)
    for gp in gps:
        gp._ensure_resident()
    out = eng.cnehvi_greedy(draws, q, pareto.constraints[:, 0], pareto.constraints[:, 1], pareto.ref_point,
                            base=np.ascontiguousarray(base, dtype=np.float64), y_mean=[m.y_mean for m in models],
                            y_std=[m.y_std for m in models], return_fronts=True)
    index, picks = S.picked_params(eng, out["index"], d, lambda x: dict(zip(pareto.keys, x)))
    if return_info:
        sizes = np.asarray(out["front_size"])
        return picks, {"gain": np.asarray(out["gain"], dtype=np.float64), "index": index,
                       "feasible": np.asarray(out["feasible"], dtype=np.float64),
                       "front_size_before": int(sizes[0].max()), "front_size_after": int(sizes[1].max()), "n_draws": G * n_paths}
    return picks
