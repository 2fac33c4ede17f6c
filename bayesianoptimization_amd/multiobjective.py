"""Multi-objective Bayesian optimisation by expected hypervolume improvement (EHVI; Emmerich, Giannakoglou & Naujoks 2006, "Single-
and multiobjective evolutionary optimization assisted by Gaussian random field metamodels"; the box form of Yang, Emmerich, Deutz &
Bäck 2019, "Efficient computation of expected hypervolume improvement using box decomposition algorithms").

All m = 2 or 3 objectives are MAXIMISED, in raw target units.  Objective j has its own GP in slot j of one engine; the posteriors
are independent.  For a reference point r and the non-dominated front P of the observations, the region above r that P does not
dominate is cut into K disjoint boxes [l_k, u_k) whose bounds are entries of per-objective level lists (r_j, the distinct front
values, +inf), and

    g_j(a)  = E[(Y_j - a)^+] = sd_j f((mu_j - a) / sd_j),   f(z) = phi(z) + z Phi(z),   g_j(+inf) = 0
    EHVI(x) = sum_k prod_j (g_j(l_kj) - g_j(u_kj))

is the expected growth of the dominated hypervolume from observing x.  The values come from ONE posterior pass per objective over
one candidate set plus the sum over the boxes (the engine's `ehvi_argbest`, gpbo_ehvi_argbest; include/gpbo.h has the ranges f is
evaluated over, the conventions and the order of the sum).

`pareto_front`, `hypervolume` and `box_decomposition` are the host side: plain NumPy, no device.

Black-box constraints: `ParetoOptimizer(..., constraints=[(lb, ub), ...])` gives every constraint a GP of its own in the slots behind
the objectives', keeps `front` and `hypervolume` to the FEASIBLE observations, and `suggest` weights the EHVI by the probability
that every constraint holds, in log form: log EHVI(x) + sum_j log p_j(x) (the engine's `cehvi_argbest`, gpmo_cehvi_argbest;
include/gpmo.h has the formulas).

Out of scope here: m > 3, a local-search stage.  Batches of q > 1 points and the noisy-front variant (NEHVI) are `suggest_qnehvi`
(qnehvi.py) and, under constraints, `suggest_constrained_qnehvi` (cqnehvi.py), both for m = 2; for m = 3 they are out of scope too.
"""
from __future__ import annotations

import contextlib
import warnings

import numpy as np

from ._lib import MAX_EHVI_CELLS, MAX_EHVI_LEVELS, MAX_EHVI_OBJECTIVES, MAX_MODELS

#: the largest front `ParetoOptimizer.suggest` serves: GPBO_MAX_EHVI_LEVELS less r_j and +inf
MAX_FRONT = MAX_EHVI_LEVELS - 2


def _points(Y, ref_point):
    ref = np.asarray(ref_point, dtype=np.float64).ravel()
    Y = np.asarray(Y, dtype=np.float64)
    Y = Y.reshape(-1, ref.shape[0]) if Y.size == 0 else np.atleast_2d(Y)
    if Y.ndim != 2 or Y.shape[1] != ref.shape[0]:
        raise ValueError("Y must be (n, m) with m the length of ref_point")
    return Y, ref


def pareto_front(Y, ref_point):
    """The rows of Y (n, m) that are strictly above `ref_point` in every objective and not dominated (no other row is >= everywhere
    and > somewhere), all objectives maximised.  Equal rows are kept once; the order is that of first appearance."""
    Y, ref = _points(Y, ref_point)
    Y = Y[np.all(Y > ref, axis=1)]
    if Y.shape[0] == 0:
        return Y
    _, first = np.unique(Y, axis=0, return_index=True)
    Y = Y[np.sort(first)]
    ge = np.all(Y[:, None, :] >= Y[None, :, :], axis=2)       # ge[a, b]: row a >= row b everywhere
    gt = np.any(Y[:, None, :] > Y[None, :, :], axis=2)
    return Y[~np.any(ge & gt, axis=0)]


def _hv2(P, ref):
    """Area dominated by the rows of P (n, 2), all strictly above ref."""
    if P.shape[0] == 0:
        return 0.0
    P = P[np.lexsort((-P[:, 1], -P[:, 0]))]                  # objective 0 descending
    area, top = 0.0, ref[1]
    for a, b in P:
        if b > top:
            area += (a - ref[0]) * (b - top)
            top = b
    return float(area)


def hypervolume(Y, ref_point):
    """The exact hypervolume dominated by the rows of Y (n, m) above `ref_point`, m = 2 or 3, all objectives maximised: the measure
    of the union of the boxes [ref_point, y).  Rows not strictly above the reference point contribute nothing."""
    Y, ref = _points(Y, ref_point)
    m = ref.shape[0]
    if m not in (2, 3):
        raise ValueError("hypervolume: 2 or 3 objectives")
    P = pareto_front(Y, ref)
    if m == 2:
        return _hv2(P, ref)
    # slices along objective 2, from the top: between two consecutive heights the cross-section is the area of the rows at or above
    heights = np.unique(P[:, 2])[::-1]
    total = 0.0
    for i, h in enumerate(heights):
        below = heights[i + 1] if i + 1 < heights.shape[0] else ref[2]
        total += (h - below) * _hv2(P[P[:, 2] >= h][:, :2], ref[:2])
    return float(total)


def box_decomposition(front, ref_point):
    """The region above `ref_point` that `front` (n, m; non-dominated, strictly above the reference point: `pareto_front`'s result)
    does not dominate, as disjoint boxes: (n_levels (m,), levels (m, GPBO_MAX_EHVI_LEVELS), cell_lo (K, m), cell_hi (K, m)) as
    `GpEngine.ehvi_argbest` takes them.

    Row j of `levels` holds r_j, the distinct values of objective j on the front in increasing order, and +inf (and +inf as
    padding); cell_lo / cell_hi index into it, box k = prod_j [levels[j, lo_kj], levels[j, hi_kj]).  The grid form: one box per cell
    of the grid over objectives 0 .. m - 2, whose bounds there are ADJACENT levels; its lower bound in objective m - 1 is the largest
    value of that objective among the front points that are >= the box's upper bound in every other objective (r_{m-1} without
    one), its upper bound +inf.  K = prod_{j < m-1} (n_levels[j] - 1); an empty front gives the one box [r, +inf)."""
    front, ref = _points(front, ref_point)
    m = ref.shape[0]
    if not 2 <= m <= MAX_EHVI_OBJECTIVES:
        raise ValueError("box_decomposition: 2 or 3 objectives")
    if not np.all(np.isfinite(ref)) or not np.all(np.isfinite(front)):
        raise ValueError("box_decomposition: ref_point and front must be finite")
    if front.shape[0] and not np.all(front > ref):
        raise ValueError("box_decomposition: the front must be strictly above ref_point in every objective")
    rows = [np.concatenate([[ref[j]], np.unique(front[:, j]), [np.inf]]) for j in range(m)]
    n_levels = np.array([r.shape[0] for r in rows], dtype=np.int64)
    if n_levels.max() > MAX_EHVI_LEVELS:
        raise ValueError(f"box_decomposition: more than {MAX_FRONT} distinct front values in one objective")
    levels = np.full((m, MAX_EHVI_LEVELS), np.inf)
    for j, r in enumerate(rows):
        levels[j, :r.shape[0]] = r
    grid = [np.arange(n - 1) for n in n_levels[:-1]]
    idx = np.stack(np.meshgrid(*grid, indexing="ij"), axis=-1).reshape(-1, m - 1)      # (K, m - 1) lower level indices
    K = idx.shape[0]
    assert K <= MAX_EHVI_CELLS
    # covers[k, p]: front point p is >= box k's upper bound in every objective but the last
    covers = np.ones((K, front.shape[0]), dtype=bool)
    for j in range(m - 1):
        covers &= front[None, :, j] >= rows[j][idx[:, j] + 1][:, None]
    floor = np.where(covers, front[None, :, m - 1], ref[m - 1]).max(axis=1, initial=ref[m - 1])
    cell_lo = np.empty((K, m), dtype=np.int64)
    cell_hi = np.empty((K, m), dtype=np.int64)
    cell_lo[:, :m - 1], cell_hi[:, :m - 1] = idx, idx + 1
    cell_lo[:, m - 1] = np.searchsorted(rows[m - 1], floor)
    cell_hi[:, m - 1] = n_levels[m - 1] - 1
    return n_levels, levels, cell_lo, cell_hi


class ParetoOptimizer:
    """Multi-objective Bayesian optimisation over an all-float box by EHVI: `register` observations, `suggest` the next point,
    read `front` and `hypervolume`.  Needs no bayes_opt.

    `pbounds`: {name: (lo, hi)}; `n_objectives` m = 2 or 3, all maximised; `ref_point` (m,) the hypervolume's reference point, raw
    target units — a point every acceptable outcome is above.  It owns m `HipGPR`s, objective j in slot j of ONE engine (`engine`,
    or the process's shared engine of `device`), built with the defaults `accelerate()` leaves a `BayesianOptimization` with:
    Matern(nu=2.5) (or a clone of `kernel` each), `alpha`, `normalize_y=True`, `n_restarts_optimizer`, and one RandomState
    (`random_state`) shared by the theta searches and the candidate draws.  `flags`: `matern_family` / `scaled_kernels` /
    `scaled_lanes` / `precision`, passed to every HipGPR.

    `constraints`: None, or a sequence of C (lb, ub) pairs, lb < ub, infinite sides allowed, m + C <= 8: black-box constraints
    c_j(x) that hold where lb_j <= c_j(x) <= ub_j.  Constraint j gets a HipGPR of the objectives' construction in slot m + j;
    `register` then takes the C measured constraint values too, `feasible` is the mask of the observations whose measured values
    hold, `front` and `hypervolume` are over those alone, and `suggest` weights the EHVI by the feasibility (below).

    Out of scope: m > 3, a local-search stage — the pick is among the candidates.  Batches of q > 1 points and the noisy-front
    variant (NEHVI): `suggest_qnehvi(self, q)` — with constraints `suggest_constrained_qnehvi(self, q)` — for m = 2, out of scope
    for m = 3."""

    _FLAGS = ("matern_family", "scaled_kernels", "scaled_lanes", "precision")

    def __init__(self, pbounds, n_objectives, ref_point, kernel=None, alpha=1e-6, n_restarts_optimizer=5, random_state=None,
                 engine=None, device=0, constraints=None, **flags):
        from sklearn.base import clone
        from sklearn.gaussian_process.kernels import Matern

        from .float_space import ensure_rng
        from .gpr import HipGPR

        if isinstance(n_objectives, bool) or not isinstance(n_objectives, (int, np.integer)) \
                or not 2 <= n_objectives <= MAX_EHVI_OBJECTIVES:
            raise ValueError(f"n_objectives must be an integer in [2, {MAX_EHVI_OBJECTIVES}]")
        unknown = set(flags) - set(self._FLAGS)
        if unknown:
            raise TypeError(f"ParetoOptimizer: unknown flags {sorted(unknown)}")
        self.n_objectives = int(n_objectives)
        self.ref_point = np.array(ref_point, dtype=np.float64).ravel()
        if self.ref_point.shape[0] != self.n_objectives or not np.all(np.isfinite(self.ref_point)):
            raise ValueError("ref_point must hold one finite value per objective")
        self.keys = list(pbounds.keys())
        self.bounds = np.array([[float(lo), float(hi)] for lo, hi in pbounds.values()], dtype=np.float64)
        if self.bounds.shape[0] < 1 or not np.all(self.bounds[:, 0] < self.bounds[:, 1]):
            raise ValueError("pbounds must give lo < hi for at least one parameter")
        self.constraints = None
        if constraints is not None:
            try:
                pairs = np.array([[float(lo), float(hi)] for lo, hi in constraints], dtype=np.float64).reshape(-1, 2)
            except (TypeError, ValueError):
                raise ValueError("constraints must be a sequence of (lb, ub) pairs") from None
            if pairs.shape[0] < 1 or np.isnan(pairs).any() or not np.all(pairs[:, 0] < pairs[:, 1]):
                raise ValueError("constraints must be at least one (lb, ub) pair, without a NaN and with lb < ub")
            if self.n_objectives + pairs.shape[0] > MAX_MODELS:
                raise ValueError(f"n_objectives + the number of constraints must not exceed {MAX_MODELS}, the engine's model slots")
            self.constraints = pairs
        self._random_state = ensure_rng(random_state)
        self._engine_arg, self._device = engine, device
        self._params = np.empty((0, self.bounds.shape[0]))
        self._targets = np.empty((0, self.n_objectives))
        self._gps = [HipGPR(kernel=Matern(nu=2.5) if kernel is None else clone(kernel), alpha=alpha, normalize_y=True,
                            n_restarts_optimizer=n_restarts_optimizer, random_state=self._random_state, engine=engine, slot=j,
                            **flags) for j in range(self.n_objectives)]
        n_c = 0 if self.constraints is None else self.constraints.shape[0]
        self._constraint_values = np.empty((0, n_c))
        self._cgps = [HipGPR(kernel=Matern(nu=2.5) if kernel is None else clone(kernel), alpha=alpha, normalize_y=True,
                             n_restarts_optimizer=n_restarts_optimizer, random_state=self._random_state, engine=engine,
                             slot=self.n_objectives + j, **flags) for j in range(n_c)]

    # -- the store ------------------------------------------------------------------------------------------------------------
    def __len__(self):
        return self._targets.shape[0]

    @property
    def params(self):
        return self._params

    @property
    def targets(self):
        return self._targets

    @property
    def constraint_values(self):
        """(n, C) the measured constraint values ((n, 0) without constraints)"""
        return self._constraint_values if self.constraints is not None else np.empty((len(self), 0))

    def register(self, params, targets, constraint_values=None):
        """One observation: `params` a {name: value} dict or a (d,) array in `pbounds`' order, `targets` (m,) finite values; with
        `constraints`, `constraint_values` (C,) the finite measured values of the constraints (without: None)."""
        if isinstance(params, dict):
            if set(params) != set(self.keys):
                raise ValueError(f"params must have exactly the keys {self.keys}")
            x = np.array([params[k] for k in self.keys], dtype=np.float64)
        else:
            x = np.asarray(params, dtype=np.float64).ravel()
        y = np.asarray(targets, dtype=np.float64).ravel()
        if x.shape[0] != self.bounds.shape[0] or not np.all(np.isfinite(x)):
            raise ValueError("params must hold one finite value per parameter")
        if y.shape[0] != self.n_objectives or not np.all(np.isfinite(y)):
            raise ValueError("targets must hold one finite value per objective")
        if self.constraints is None:
            if constraint_values is not None:
                raise ValueError("constraint_values given, but the optimizer has no constraints")
        else:
            c = np.empty(0) if constraint_values is None else np.asarray(constraint_values, dtype=np.float64).ravel()
            if c.shape[0] != self.constraints.shape[0] or not np.all(np.isfinite(c)):
                raise ValueError("constraint_values must hold one finite value per constraint")
            self._constraint_values = np.concatenate([self._constraint_values, c[None]])
        self._params = np.concatenate([self._params, x[None]])
        self._targets = np.concatenate([self._targets, y[None]])

    @property
    def feasible(self):
        """(n,) bool: the observations whose measured constraint values all lie in their [lb, ub]; all True without constraints."""
        if self.constraints is None:
            return np.ones(len(self), dtype=bool)
        c = self._constraint_values
        return np.all((c >= self.constraints[:, 0]) & (c <= self.constraints[:, 1]), axis=1)

    def _feasible_observations(self):
        """(params, targets) of the feasible observations: all of them without constraints"""
        if self.constraints is None:
            return self._params, self._targets
        ok = self.feasible
        return self._params[ok], self._targets[ok]

    @property
    def front(self):
        """(params (k, d), targets (k, m)) of the non-dominated observations strictly above `ref_point` (`pareto_front`: equal
        targets once, at their first observation; order of first appearance).  With `constraints`: of the FEASIBLE observations."""
        params, targets = self._feasible_observations()
        P = pareto_front(targets, self.ref_point)
        rows = [int(np.flatnonzero(np.all(targets == p, axis=1))[0]) for p in P]
        return params[rows], P

    @property
    def hypervolume(self):
        """The hypervolume the observations dominate above `ref_point`.  With `constraints`: the FEASIBLE observations."""
        return hypervolume(self._feasible_observations()[1], self.ref_point)

    # -- the suggestion -------------------------------------------------------------------------------------------------------
    def _engine(self):
        if self._engine_arg is None:
            from .gpr import shared_engine

            self._engine_arg = shared_engine(self._device)
            for gp in self._gps + self._cgps:
                gp.engine = self._engine_arg
        return self._engine_arg

    def _constraint_host_reason(self):
        """(j, reason) of the first constraint whose model would run on the host, else None"""
        from sklearn.base import clone

        for j, gp in enumerate(self._cgps):
            reason = gp._unsupported_reason(clone(gp.kernel), self._constraint_values[:, j], self._params)
            if reason is not None:
                return j, reason
        return None

    def suggest(self, n_random: int = 10_000, return_info: bool = False):
        """One parameter dict to probe next: the candidate of the largest expected hypervolume improvement.  In this order:

          1. the argument check (ValueError: `n_random` not an integer >= 1).
          2. the refusals, in this order: TargetSpaceEmptyError on an empty store; NotImplementedError — never a host fallback, never
             a thinned front — for a device group, for an objective whose model would run on the host, and for a front of more than
             128 points.
          3. the m fits on the observations in slot order 0 .. m - 1, overlapped on the device where the engine can, warnings
             silenced.  Each fit's theta search draws its restarts' starting points from the RandomState: objective 0's
             n_restarts_optimizer draws first, then objective 1's, ...
          4. ONE candidate draw of `n_random` points from the RandomState, on the device: the state advances as
             d calls of uniform(lo_t, hi_t, n_random) would advance it.
          5. one posterior pass per objective, in slot order, left on the device.
          6. `ehvi_argbest` over the boxes of `box_decomposition(front, ref_point)`.
          7. the picked row is fetched from the device.
        Nothing else draws from the RandomState.  `return_info=True`: (params, info), info = {"value": the pick's EHVI, "index": its
        candidate index, "n_cells": K, "front_size": the front's size}.

        With `constraints` (C of them) the same order, and in addition: in 2. NotImplementedError for an engine without
        `cehvi_argbest` and for a constraint whose model would run on the host, and the front is the FEASIBLE observations'; in 3.
        the C constraint fits follow the objectives' in slot order m .. m + C - 1, their theta searches' draws after the
        objectives', in slot order; in 5. their posterior passes follow too; 6. is `cehvi_argbest` in log form over the boxes of the
        feasible front — none feasible yet: the one box [r, +inf), "improve on r, weighted by feasibility" —, and info["value"] is
        log EHVI + sum_j log p_j at the pick.

        Out of scope: m > 3, a local-search stage (the pick is AMONG THE CANDIDATES); q > 1 and NEHVI are `suggest_qnehvi` /
        `suggest_constrained_qnehvi` for m = 2."""
        from sklearn.base import clone

        from . import fused_acquisition as A
        from .engine import GroupEngine

        if isinstance(n_random, bool) or not isinstance(n_random, (int, np.integer)) or n_random < 1:
            raise ValueError("n_random must be an integer >= 1")
        n_random = int(n_random)
        if len(self) == 0:
            raise A.TargetSpaceEmptyError(A.EMPTY_SPACE_MESSAGE)
        eng = self._engine()
        if isinstance(eng, GroupEngine):
            raise NotImplementedError("ParetoOptimizer.suggest: a device group has no expected hypervolume improvement; "
                                      "use a single device")
        for j, gp in enumerate(self._gps):
            reason = gp._unsupported_reason(clone(gp.kernel), self._targets[:, j], self._params)
            if reason is not None:
                raise NotImplementedError(f"ParetoOptimizer.suggest: objective {j}'s model runs on the host ({reason}); only models "
                                          "on the device path are served")
        if self.constraints is not None:
            if not hasattr(eng, "cehvi_argbest"):
                raise NotImplementedError("ParetoOptimizer.suggest: the engine has no cehvi_argbest")
            host = self._constraint_host_reason()
            if host is not None:
                raise NotImplementedError(f"ParetoOptimizer.suggest: constraint {host[0]}'s model runs on the host ({host[1]}); only "
                                          "models on the device path are served")
        P = pareto_front(self._feasible_observations()[1], self.ref_point)
        if P.shape[0] > MAX_FRONT:
            raise NotImplementedError(f"ParetoOptimizer.suggest: the front has {P.shape[0]} points, more than the {MAX_FRONT} "
                                      "gpbo_ehvi_argbest's level lists hold; the front is never thinned")
        overlap = eng.overlapped_fits() if hasattr(eng, "overlapped_fits") else contextlib.nullcontext()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with overlap:
                for j, gp in enumerate(self._gps):
                    gp.fit(self._params, self._targets[:, j])
                for j, gp in enumerate(self._cgps):
                    gp.fit(self._params, self._constraint_values[:, j])
        if any(gp._host_mode for gp in self._gps + self._cgps):      # (unreachable after the refusals; a host model must not get this far silently)
            raise NotImplementedError("ParetoOptimizer.suggest: a model was fitted on the host")
        eng.generate_candidates_like(n_random, self.bounds[:, 0], self.bounds[:, 1], self._random_state)
        for gp in self._gps + self._cgps:
            gp._ensure_resident()
            eng.posterior(slot=gp.slot, y_mean=float(gp._y_train_mean), y_std=float(gp._y_train_std), fetch=False)
        _n_levels, levels, cell_lo, cell_hi = box_decomposition(P, self.ref_point)
        if self.constraints is None:
            index, value, _seed_idx, _seed_val, _ys = eng.ehvi_argbest(levels, cell_lo, cell_hi)
        else:
            index, value, _seed_idx, _seed_val, _ys = eng.cehvi_argbest(levels, cell_lo, cell_hi, self.constraints[:, 0],
                                                                        self.constraints[:, 1], log_form=True)
        row = np.asarray(eng.get_candidate_rows(np.array([index], dtype=np.int64), self.bounds.shape[0]), dtype=np.float64)[0]
        params = dict(zip(self.keys, row))
        if return_info:
            return params, {"value": -float(value), "index": int(index), "n_cells": int(cell_lo.shape[0]),
                            "front_size": int(P.shape[0])}
        return params
