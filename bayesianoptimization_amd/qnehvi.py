"""suggest_qnehvi(pareto, q) — q points to probe in parallel for TWO noisy objectives, by batch noisy expected hypervolume
improvement (qNEHVI; Daulton, Balandat & Bakshy 2021, "Parallel Bayesian optimization of multiple noisy objectives with expected
hypervolume improvement"), in its greedy, cached-draws form.

`ParetoOptimizer.suggest` scores candidates against the front of the raw observations and hands out one point.  With observation
noise that front is itself noisy — a lucky reading sits on it and the improvement is measured against a phantom.  Here T joint
draws (f0_t, f1_t) of the two LATENT objectives are taken from the posteriors (the pathwise-conditioned draws of thompson.py, one
independent GP per objective), and each draw brings a Pareto front of its own: the non-dominated set of the draw's values at the
points already observed — and at points still pending.  A candidate is worth the mean over the draws of the hypervolume it adds,

    a(x) = 1/T sum_t HVI((f0_t(x), f1_t(x)) | P_t),

and a batch is built greedily: after a pick every draw's front absorbs the draw's values there, so the next pick is scored JOINTLY
with the earlier ones — no made-up observation, no refit.  The whole loop is ONE engine call (`qnehvi_greedy`, gpbo_qnhvi_greedy;
include/gpbo.h has the formulas and the conventions): the draws stay on the device as a (2, T, M) block, the fronts are built
there, and the q scoring passes, selections and front updates run on the stream without a host round trip.

m = 2 only: at two objectives a front is a staircase and the improvement a sum over its strips.  Three objectives need a box
decomposition per draw on the device; they are refused, not approximated.  Black-box constraints are served by
`suggest_constrained_qnehvi` (cqnehvi.py), which masks objective 0's draw by the draw's own constraint draws; this function scores
fronts built from every observed point and refuses nothing on their account.
"""
from __future__ import annotations

import contextlib
import warnings

import numpy as np

from . import _suggest as S
from ._lib import MAX_QNEHVI_BASE as MAX_BASE


def suggest_qnehvi(pareto, q: int, n_random: int = 10_000, n_draws: int = 64, n_features: int = 1024, pending=None,
                   return_info: bool = False):
    """q parameter dicts to probe side by side for the two objectives of `pareto`, a `ParetoOptimizer`.  In this order:

      1. the argument checks (ValueError, below).
      2. the refusals: NotImplementedError for `n_objectives == 3`; then `ParetoOptimizer.suggest`'s — TargetSpaceEmptyError on
         an empty store, NotImplementedError (never a host fallback) for a device group and for an objective whose model would
         run on the host.  ValueError when the observed and the pending points together exceed 16384.
      3. the two fits on the observations in slot order, overlapped on the device where the engine can, warnings silenced; each
         fit's theta search draws from the RandomState, objective 0's first.
      4. ONE candidate draw of `n_random` points from the RandomState, on the device, as `suggest` draws it.
      5. objective 0's G groups of S posterior draws, then objective 1's (`draw_layout`: G = ceil(n_draws / 16), S = ceil(n_draws /
         G), T = G * S >= n_draws; info["n_draws"] says how many).  Each group draws from the RandomState as `suggest_qnei`'s —
         `spectral_draw` for the objective's kernel (fresh features per group), `standard_normal((S, F))`, `standard_normal((S,
         N))` scaled by sqrt(noise), the noise that objective's alpha (+ its WhiteKernel's level).
      6. ONE `qnehvi_greedy` call with `base` = the observed params followed by `pending` (a list of parameter dicts or an array
         (P, d): points suggested but not yet observed): the draws, every draw's front, and the q greedy picks.
      7. the picked rows are fetched from the device.
    Nothing else draws from the RandomState.  No posterior pass, no local search: the picks are AMONG THE CANDIDATES.  Once no
    candidate adds hypervolume to any draw's front the best gain is exactly 0 and the device's rule (ties to the lowest index) hands
    out the lowest unpicked index, a uniform random point; such a pick is kept and reported, info["gain"] is 0 there.
    `return_info=True`: (picks, info), info = {"gain": (q,) each pick's gain when it was picked, "index": (q,) the candidate
    indices, "front_size_before" / "front_size_after": the largest front of any draw before the first pick / after the last,
    "n_draws": T}.

    ValueError: q not an integer in [1, 64] (or larger than `n_random`), n_random < 1, n_draws not an integer in [1, 256],
    n_features outside [1, 4096], pending of another shape or not finite.  NotImplementedError also when a draw's front outgrows
    128 points (gpbo_qnhvi_greedy never thins a front)."""
    who = "suggest_qnehvi"
    q, n_random, n_draws, n_features = S.greedy_counts(q, n_random, n_draws, n_features)
    d = int(pareto.bounds.shape[0])
    pending = S.pending_rows(pending, pareto, d)
    if pareto.n_objectives != 2:
        raise NotImplementedError(f"{who}: {pareto.n_objectives} objectives; a draw's front is a staircase for two objectives "
                                  "only (gpbo_qnhvi_greedy serves m = 2 and approximates nothing)")
    eng = S.pareto_gate(pareto, who, "batch noisy expected hypervolume improvement")
    if not hasattr(eng, "qnehvi_greedy"):
        raise NotImplementedError(f"{who}: the engine has no qnehvi_greedy")
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
    out = eng.qnehvi_greedy(draws, q, pareto.ref_point, base=np.ascontiguousarray(base, dtype=np.float64),
                            y_mean=[m.y_mean for m in models], y_std=[m.y_std for m in models], return_fronts=True)
    index, picks = S.picked_params(eng, out["index"], d, lambda x: dict(zip(pareto.keys, x)))
    if return_info:
        sizes = np.asarray(out["front_size"])
        return picks, {"gain": np.asarray(out["gain"], dtype=np.float64), "index": index,
                       "front_size_before": int(sizes[0].max()), "front_size_after": int(sizes[1].max()), "n_draws": G * n_paths}
    return picks
