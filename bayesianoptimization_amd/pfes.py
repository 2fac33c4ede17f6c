"""suggest_pfes(pareto) — the next point to probe for TWO objectives by Pareto-frontier entropy search (PFES; Suzuki, Takeno,
Tamura, Shitara & Karasuyama 2020, "Multi-objective Bayesian optimization using Pareto-frontier entropy"), the
information-theoretic alternative to `ParetoOptimizer.suggest`'s expected hypervolume improvement.

Hypervolume needs a reference point and is myopic about the front's shape.  PFES asks instead how much an observation at x would
tell about the Pareto front itself: S joint draws (f0_s, f1_s) of the two latent objectives are taken from the posteriors (the
pathwise-conditioned draws of thompson.py, one independent GP per objective), each draw brings a Pareto front F_s of its own — the
non-dominated set of the draw's values over the candidates —, and a candidate is worth

    a(x) = 1/S sum_s ( H[p(y | x)] - H[p(y | x, y dominated by F_s)] ),

the entropy its observation loses once it is known to lie under the sampled front.  For two objectives the dominated region is a
union of strips under a staircase and both entropies are closed forms in Phi and phi (include/gppf.h).  The draws, the fronts, the
score of every candidate and the selection are ONE engine call (`pfes_argbest`, gppf_pfes_argbest).  No reference point enters:
`pareto.ref_point` is not looked at.

m = 2 only: three objectives need a box decomposition of every sampled front and are refused, as are black-box constraints.
"""
from __future__ import annotations

import contextlib
import warnings

import numpy as np

from . import _suggest as S
from ._lib import MAX_PATH_FEATURES
from ._lib import MAX_PFES_SAMPLES as MAX_SAMPLES


def suggest_pfes(pareto, n_random: int = 10_000, n_samples: int = 16, n_features: int = 1024, return_info: bool = False):
    """One parameter dict to probe next for the two objectives of `pareto`, a `ParetoOptimizer`.  In this order:

      1. the argument checks (ValueError, below).
      2. the refusals: NotImplementedError for `n_objectives == 3` and for a constrained optimizer; then
         `ParetoOptimizer.suggest`'s — TargetSpaceEmptyError on an empty store, NotImplementedError (never a host fallback) for a
         device group and for an objective whose model would run on the host.
      3. the two fits on the observations in slot order, overlapped on the device where the engine can, warnings silenced; each
         fit's theta search draws from the RandomState, objective 0's first.
      4. ONE candidate draw of `n_random` points from the RandomState, on the device, as `suggest` draws it.
      5. one posterior pass per objective, in slot order, left on the device (they draw nothing).
      6. objective 0's G groups of S posterior draws, then objective 1's (`draw_layout`: G = ceil(n_samples / 16), S =
         ceil(n_samples / G), G * S >= n_samples; info["n_samples"] says how many).  Each group draws from the RandomState as
         `suggest_qnehvi`'s — `spectral_draw` for the objective's kernel (fresh features per group), `standard_normal((S, F))`,
         `standard_normal((S, N))` scaled by sqrt(noise), the noise that objective's alpha (+ its WhiteKernel's level).
      7. ONE `pfes_argbest` call: every joint draw's front over the first min(n_random, 16384) candidates, the score of every
         candidate, the selection.
      8. the picked row is fetched from the device.
    Nothing else draws from the RandomState.  No local search: the pick is AMONG THE CANDIDATES.
    `return_info=True`: (params, info), info = {"value": the pick's a(x) in nats, "index": its candidate index, "front_size": (G S,)
    the sampled fronts' sizes, "n_samples": G S}.

    ValueError: n_random not an integer >= 1, n_samples not an integer in [1, 64], n_features outside [1, 4096].
    NotImplementedError also when a sampled front outgrows 128 points (gppf_pfes_argbest never thins a front)."""
    who = "suggest_pfes"
    n_random = S.count(n_random, 1, None, "n_random must be an integer >= 1")
    n_samples = S.count(n_samples, 1, MAX_SAMPLES, f"n_samples must be an integer in [1, {MAX_SAMPLES}]")
    n_features = int(n_features)
    if not 1 <= n_features <= MAX_PATH_FEATURES:
        raise ValueError(f"n_features must be in [1, {MAX_PATH_FEATURES}]")
    if pareto.n_objectives != 2:
        raise NotImplementedError(f"{who}: {pareto.n_objectives} objectives; the dominated region is a union of strips for two "
                                  "objectives only (gppf_pfes_argbest serves m = 2 and approximates nothing)")
    if pareto.constraints is not None:
        raise NotImplementedError(f"{who}: the optimizer has constraints; Pareto-frontier entropy search here is unconstrained")
    eng = S.pareto_gate(pareto, who, "Pareto-frontier entropy search")
    if not hasattr(eng, "pfes_argbest"):
        raise NotImplementedError(f"{who}: the engine has no pfes_argbest")
    rng = pareto._random_state
    d = int(pareto.bounds.shape[0])

    overlap = eng.overlapped_fits() if hasattr(eng, "overlapped_fits") else contextlib.nullcontext()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with overlap:
            for j, gp in enumerate(pareto._gps):
                gp.fit(pareto.params, pareto.targets[:, j])
    models = [S.read_model(gp, pareto, who) for gp in pareto._gps]
    eng.generate_candidates_like(n_random, pareto.bounds[:, 0], pareto.bounds[:, 1], rng)
    for gp, model in zip(pareto._gps, models):
        gp._ensure_resident()
        eng.posterior(slot=gp.slot, y_mean=model.y_mean, y_std=model.y_std, fetch=False)
    G, n_paths = S.draw_layout(n_samples)
    draws = [S.group_inputs(gp, rng, model, G, n_paths, n_features) for gp, model in zip(pareto._gps, models)]
    index, value, _seed_idx, _seed_val, _ys, front_size, _fronts = eng.pfes_argbest(
        draws=draws, y_mean=[m.y_mean for m in models], y_std=[m.y_std for m in models], return_fronts=True)
    index, picks = S.picked_params(eng, [index], d, lambda x: dict(zip(pareto.keys, x)))
    if return_info:
        return picks[0], {"value": -float(value), "index": int(index[0]), "front_size": np.asarray(front_size), "n_samples": G * n_paths}
    return picks[0]
