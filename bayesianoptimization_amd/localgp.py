"""suggest_local(optimizer) — the next point to probe when the optimizer holds 10^4 .. 10^6 observations: nearest-neighbour GP
scoring (Vecchia 1988, "Estimation and model identification for continuous spatial processes"; Emery 2009, "The kriging update
equations and their application to the selection of neighboring data"; Datta, Banerjee, Finley & Gelfand 2016, "Hierarchical
nearest-neighbor Gaussian process models for large geostatistical datasets"; Gramacy & Apley 2015, "Local Gaussian process
approximation for large computer experiments").

Every other suggest function here works on an exact GP: an O(N^3) fit and N^2 per candidate, which ends in practice at a few
thousand observations.  A cheap simulator with 20 000 or 500 000 evaluations needs another model: at FIXED hyper-parameters a
candidate's posterior is taken from the exact GP conditioned on its k nearest observations only — O(N d) for the search and O(k^3)
for a small solve per candidate, no N x N matrix anywhere (the engine's `nn_acq_argbest`, gpnn_acq_argbest; include/gpnn.h has the
formulas and the conventions).  The hyper-parameters come from the existing device fit on a random subset of the observations.
"""
from __future__ import annotations

import numpy as np

from . import _suggest as S
from . import fused_acquisition as A
from ._lib import MAX_NN_N
from .engine import EI, LOG_EI, POI, UCB

_ACQUISITIONS = {"ucb": UCB, "ei": EI, "poi": POI, "log_ei": LOG_EI}
_NEIGHBORS = (16, 32, 64)


class ConstrainedSpaceNotImplemented(A.ConstraintNotSupportedError, NotImplementedError):
    """A constrained space: the suggest functions' ConstraintNotSupportedError, and a NotImplementedError — nothing here falls back
    to the host."""


def suggest_local(optimizer, n_neighbors: int = 32, n_random: int = 100_000, theta_subset: int = 2048, acquisition: str = "ucb",
                  kappa: float = 2.576, xi: float = 0.01, return_info: bool = False):
    """One parameter dict to probe next, as `suggest` returns it; `optimizer` has been `accelerate()`d.

      1. the checks below.  The acquisition policy is neither consulted nor advanced.
      2. theta: `gp.fit`, theta search included, on at most `theta_subset` observations — all of them when N <= theta_subset, else
         the rows `sort(RandomState.choice(N, theta_subset, replace=False))`.  Slot 0 is left fitted to THAT subset.
      3. ONE candidate draw of `n_random` points, on the device.
      4. ONE `nn_acq_argbest` over all N observations at that theta — kernel kind, length scales, the estimator's alpha and, for a
         scaled model, its amplitude and white noise —, the targets normalised by the mean and standard deviation of all N (the
         deviation taken as 1 below 10 eps, as the estimator does); `acquisition` is "ucb" (`kappa`), "ei", "poi" or "log_ei" (`xi`,
         against the best observed target).  The picked row is fetched from the device.
    The pick is AMONG THE CANDIDATES: there is no local-search stage.  The optimizer's RandomState is drawn from in this order:
    the subset (`choice`, only when N > theta_subset), the theta search's restarts (`gp.fit`), the candidates (`n_random` x d
    uniforms) — and nothing else.  `return_info=True`: (params, info) with info = {"index": the pick's candidate index, "value":
    its acquisition value, "mu", "sd": its posterior in raw target units, "neighbors": the rows it was conditioned on, nearest
    first, "subset": the rows theta was fitted on}.

    ValueError: n_neighbors not 16, 32 or 64; n_random not an integer >= 1; theta_subset not an integer in [n_neighbors, 65536];
    acquisition not one of the four names; kappa / xi not a finite number; fewer than n_neighbors or more than 2^20 observations.
    TargetSpaceEmptyError on an empty space.  NotImplementedError, never a host fallback, for: a GP that is not on the engine's slot
    0, a constrained space (ConstrainedSpaceNotImplemented: also the ConstraintNotSupportedError every suggest function raises
    there), a space with an input transform (int / categorical parameters), a model in host mode, a device group."""
    if isinstance(n_neighbors, bool) or not isinstance(n_neighbors, (int, np.integer)) or int(n_neighbors) not in _NEIGHBORS:
        raise ValueError("n_neighbors must be 16, 32 or 64")
    k = int(n_neighbors)
    n_random = S.count(n_random, 1, None, "n_random must be an integer >= 1")
    theta_subset = S.count(theta_subset, k, 1 << 16, f"theta_subset must be an integer in [{k}, 65536]")
    if acquisition not in _ACQUISITIONS:
        raise ValueError(f"acquisition must be one of {sorted(_ACQUISITIONS)}")
    param = float(kappa if acquisition == "ucb" else xi)
    if not np.isfinite(param):
        raise ValueError("kappa / xi must be a finite number")
    try:
        gp, space, eng = S.gate(optimizer, "suggest_local", "scored", ("nn_acq_argbest",),
                                "a device group has no nearest-neighbour GP scoring; use a single device")
    except A.ConstraintNotSupportedError as e:
        raise ConstrainedSpaceNotImplemented(f"suggest_local: {e}") from None
    X, y = np.asarray(space.params, dtype=np.float64), np.asarray(space.target, dtype=np.float64)
    N = X.shape[0]
    if not k <= N <= MAX_NN_N:
        raise ValueError(f"suggest_local needs between n_neighbors = {k} and {MAX_NN_N} observations, the space has {N}")
    rng = optimizer._random_state

    subset = np.arange(N) if N <= theta_subset else np.sort(rng.choice(N, theta_subset, replace=False))
    space_subset = _Rows(X[subset], y[subset], space.bounds)
    model = S.fit_model(gp, space_subset, "suggest_local")
    amplitude, white = (1.0, 0.0) if model.scale is None else (float(model.scale[0]), float(model.scale[1]) / float(model.scale[0]))
    y_mean, y_std = float(np.mean(y)), float(np.std(y))
    if y_std < 10 * np.finfo(np.float64).eps:
        y_std = 1.0
    eng.generate_candidates_like(n_random, space.bounds[:, 0], space.bounds[:, 1], rng)
    index, value, _si, _sv, _ys, mu, sd, nbr = eng.nn_acq_argbest(
        X, (y - y_mean) / y_std, gp._kind, gp._ls, float(gp.alpha), k, _ACQUISITIONS[acquisition], param, float(np.max(y)),
        amplitude=amplitude, white=white, y_mean=y_mean, y_std=y_std, return_posterior=True, return_neighbors=True)
    row = np.asarray(eng.get_candidate_rows(np.array([index], dtype=np.int64), model.d), dtype=np.float64)[0]
    params = space.array_to_params(row)
    if return_info:
        return params, {"index": int(index), "value": -float(value), "mu": float(mu[index]), "sd": float(sd[index]),
                        "neighbors": nbr[index].copy(), "subset": subset}
    return params


class _Rows:
    """The subset of a space as `fit_model` reads it: `params`, `target`, `bounds`."""

    def __init__(self, params, target, bounds):
        self.params, self.target, self.bounds = params, target, bounds
