"""suggest_qnehvi3(pareto, q) — q points to probe in parallel for THREE noisy objectives, by batch noisy expected hypervolume
improvement (qNEHVI; Daulton, Balandat & Bakshy 2021), in its greedy, cached-draws form: `suggest_qnehvi` (qnehvi.py) for m = 3.

T joint draws (f0_t, f1_t, f2_t) of the three LATENT objectives are taken from the posteriors (one independent GP per objective), and
each draw brings a Pareto front of its own: the non-dominated set of the draw's values at the points already observed and at points
still pending.  A candidate is worth the mean over the draws of the hypervolume it adds, and a batch is built greedily: after a pick
every draw's front absorbs the draw's values there.  At three objectives a front is no staircase; every draw gets a box decomposition
of its own, built on the device by a height-map sweep (at most 2 n + 1 cells for n points) and rebuilt after every pick.  The whole
loop is ONE engine call (`qnehvi3_greedy`, gpmo3_nhvi_greedy; include/gpmo3.h has the rule and the conventions).

Black-box constraints are not served at m = 3, and neither is a device group.
"""
from __future__ import annotations

import contextlib
import warnings

import numpy as np

from . import _suggest as S
from ._lib import MAX_QNEHVI_BASE as MAX_BASE


def suggest_qnehvi3(pareto, q: int, n_random: int = 10_000, n_draws: int = 64, n_features: int = 1024, pending=None,
                    return_info: bool = False):
    """q parameter dicts to probe side by side for the three objectives of `pareto`, a `ParetoOptimizer`.  `suggest_qnehvi`'s seven
    steps, in its order, with the RandomState order extended to objective 2:

      1. the argument checks (ValueError), `suggest_qnehvi`'s.
      2. the refusals: NotImplementedError for `n_objectives != 3` (two objectives: use `suggest_qnehvi`) and for an optimizer with
         constraints; then `ParetoOptimizer.suggest`'s — TargetSpaceEmptyError on an empty store, NotImplementedError (never a host
         fallback) for a device group and for an objective whose model would run on the host.  ValueError when the observed and the
         pending points together exceed 16384.
      3. the three fits on the observations in slot order, overlapped where the engine can, warnings silenced.
      4. ONE candidate draw of `n_random` points from the RandomState, on the device.
      5. objective 0's G groups of S posterior draws, then objective 1's, then objective 2's (`draw_layout`), each group drawn from
         the RandomState as `suggest_qnehvi` draws it.
      6. ONE `qnehvi3_greedy` call with `base` = the observed params followed by `pending`.
      7. the picked rows are fetched from the device.
    The picks are AMONG THE CANDIDATES; the zero-gain tail of `suggest_qnehvi` applies.  `return_info=True`: (picks, info), info =
    {"gain" (q,), "index" (q,), "front_size_before" / "front_size_after": the largest front of any draw before the first pick / after
    the last, "n_draws": T}.  NotImplementedError also when a draw's front outgrows 128 points (a front is never thinned)."""
    who = "suggest_qnehvi3"
    q, n_random, n_draws, n_features = S.greedy_counts(q, n_random, n_draws, n_features)
    d = int(pareto.bounds.shape[0])
    pending = S.pending_rows(pending, pareto, d)
    if pareto.n_objectives != 3:
        raise NotImplementedError(f"{who}: {pareto.n_objectives} objectives; gpmo3_nhvi_greedy serves m = 3 only (two objectives: "
                                  "use suggest_qnehvi)")
    if getattr(pareto, "constraints", None) is not None:
        raise NotImplementedError(f"{who}: the optimizer has constraints; the constrained batch is served for two objectives only "
                                  "(suggest_constrained_qnehvi)")
    eng = S.pareto_gate(pareto, who, "three-objective batch noisy expected hypervolume improvement")
    if not hasattr(eng, "qnehvi3_greedy"):
        raise NotImplementedError(f"{who}: the engine has no qnehvi3_greedy")
    base = pareto.params if pending is None else np.concatenate([pareto.params, pending])
    if base.shape[0] > MAX_BASE:
        raise ValueError(f"the observed and the pending points together must not exceed {MAX_BASE}")
    rng = pareto._random_state

    overlap = eng.overlapped_fits() if hasattr(eng, "overlapped_fits") else contextlib.nullcontext()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with overlap:
            for j, gp in enumerate(pareto._gps):
                gp.fit(pareto.params, pareto.targets[:, j])
    models = [S.read_model(gp, pareto, who) for gp in pareto._gps]
    eng.generate_candidates_like(n_random, pareto.bounds[:, 0], pareto.bounds[:, 1], rng)
    G, n_paths = S.draw_layout(n_draws)
    draws = [S.group_inputs(gp, rng, model, G, n_paths, n_features) for gp, model in zip(pareto._gps, models)]
    for gp in pareto._gps:
        gp._ensure_resident()
    out = eng.qnehvi3_greedy(draws, q, pareto.ref_point, base=np.ascontiguousarray(base, dtype=np.float64),
                             y_mean=[m.y_mean for m in models], y_std=[m.y_std for m in models], return_fronts=True)
    index, picks = S.picked_params(eng, out["index"], d, lambda x: dict(zip(pareto.keys, x)))
    if return_info:
        sizes = np.asarray(out["front_size"])
        return picks, {"gain": np.asarray(out["gain"], dtype=np.float64), "index": index,
                       "front_size_before": int(sizes[0].max()), "front_size_after": int(sizes[1].max()), "n_draws": G * n_paths}
    return picks
