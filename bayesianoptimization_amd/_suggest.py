"""What suggest_batch (batch.py), suggest_thompson (thompson.py), suggest_mes (mes.py), suggest_kg (kg.py), suggest_turbo (turbo.py),
the greedy draw batches suggest_qnei (qnei.py: the gate, the frame of a model), suggest_qnehvi (qnehvi.py: `pareto_gate`, the frame of
a model) and suggest_constrained_qnei (cqnei.py: the gate with `constrained=True`) — which share `greedy_counts` (their count
checks), `draw_layout` / `MAX_DRAWS`, `pending_rows`, `group_inputs` (the draws of one model's groups, or of several models'
group-major) and `picked_params` (their tail) — and
the constrained pair suggest_constrained_thompson / suggest_scbo (scbo.py: the gate with `constrained=True`, the frame of a model)
share, each thing once: the check of a count argument, the gate an optimizer passes before anything runs, the frame of the fitted
model, the loop over groups of posterior draws, and the picks of a Thompson batch (suggest_thompson, suggest_turbo).  The ORDER of the refusals is part of the three functions' contract: a caller's own argument checks come
first, then `gate`, then whatever it checks about `refine` — so an un-accelerated optimizer is refused as such, whatever else is
wrong with the call.
"""
from __future__ import annotations

import warnings
from collections import namedtuple

import numpy as np

from . import fused_acquisition as A
from ._lib import MAX_PATH_FEATURES, MAX_PATHS, MAX_QNEI_GROUPS, MAX_SEEDS
from .engine import GroupEngine
from .gpr import HipGPR


def count(value, lo: int, hi, message: str, out_of_range=None) -> int:
    """`value` as an int if it is an integer (a bool is none) in [lo, hi] (hi None: no upper end), else ValueError(message) — an
    integer outside the range says `out_of_range` where that is given."""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise ValueError(message)
    value = int(value)
    if value < lo or (hi is not None and value > hi):
        raise ValueError(message if out_of_range is None else out_of_range)
    return value


def gate(optimizer, who: str, word: str, calls, group: str, constrained: bool = False):
    """(gp, space, engine) of an optimizer whose model `who` can work on, else the refusal — in this order: the GP is not a HipGPR on
    slot 0, the space is empty, it has a constraint, it has an input transform, the engine is a device group (`group`: the sentence
    that says what a group lacks), the engine lacks one of `calls`, the model runs on the host.  `word`: "sampled" / "batched".
    `constrained`: a constraint is admitted instead of refused, and checked LAST (`admit_constraint`)."""
    gp, space = optimizer._gp, optimizer._space
    if not isinstance(gp, HipGPR) or gp.slot != 0:
        raise NotImplementedError(f"{who}: the optimizer's GP is not on the engine (call accelerate(optimizer) first)")
    if len(space) == 0:
        raise A.TargetSpaceEmptyError(A.EMPTY_SPACE_MESSAGE)
    if space.constraint is not None and not constrained:
        raise A.ConstraintNotSupportedError(f"Received constraints, but {who} does not support constrained optimization.")
    if gp.transform is not None:
        raise NotImplementedError(f"{who}: the space has an input transform (int / categorical parameters); "
                                  f"only all-float spaces are {word}")
    eng = gp._engine()
    if isinstance(eng, GroupEngine):
        raise NotImplementedError(f"{who}: {group}")
    if not all(hasattr(eng, call) for call in calls):
        raise NotImplementedError(f"{who}: the engine has no {' / '.join(calls)}")
    from sklearn.base import clone

    reason = None if gp.kernel is None else gp._unsupported_reason(clone(gp.kernel), space.target, space.params)
    if reason is not None:
        raise NotImplementedError(f"{who}: the model runs on the host ({reason}); only models on the device path are {word}")
    if space.constraint is not None:
        admit_constraint(space, eng, who, word)
    return gp, space, eng


def admit_constraint(space, eng, who: str, word: str):
    """The constraint model of `space` as the constrained suggest functions need it, else NotImplementedError naming `who`: a
    HipConstraintModel whose GPs are HipGPRs on `eng`, constraint j in slot j (1..C), without a transform and on the device path."""
    from sklearn.base import clone

    from .constraint_model import HipConstraintModel

    cons = space.constraint
    if not isinstance(cons, HipConstraintModel):
        raise NotImplementedError(f"{who}: the space's constraint model is not a HipConstraintModel on the optimizer's engine")
    values = getattr(space, "_constraint_values", None)
    for j, cgp in enumerate(cons.model, start=1):
        if not isinstance(cgp, HipGPR) or cgp.slot != j or cgp.engine is not eng:
            raise NotImplementedError(f"{who}: constraint {j}'s GP is not on the optimizer's engine in slot {j}")
        if cgp.transform is not None:
            raise NotImplementedError(f"{who}: constraint {j}'s GP has an input transform; only all-float spaces are {word}")
        column = None if values is None else np.asarray(values).reshape(len(space), -1)[:, j - 1]
        reason = None if cgp.kernel is None or column is None else cgp._unsupported_reason(clone(cgp.kernel), column, space.params)
        if reason is not None:
            raise NotImplementedError(f"{who}: constraint {j}'s model runs on the host ({reason}); only models on the device path "
                                      f"are {word}")


#: the fitted model as the suggest functions read it.  scale: the slot's (amplitude, white), None for a unit model; noise: the
#: estimator's alpha (+ the WhiteKernel's level for a scaled model)
Model = namedtuple("Model", "d N y_mean y_std scale noise")


def read_model(gp, space, who: str) -> Model:
    """The frame of a model that has just been fitted (by `fit_model`, or by the policy's own suggest)."""
    if gp._host_mode:      # (unreachable after the gate; a host model must not get this far silently)
        raise NotImplementedError(f"{who}: the model was fitted on the host")
    scale = gp.__dict__.get("_scale")
    return Model(d=int(space.bounds.shape[0]), N=int(gp.X_train_.shape[0]), y_mean=float(gp._y_train_mean),
                 y_std=float(gp._y_train_std), scale=scale, noise=float(gp.alpha) + (0.0 if scale is None else float(scale[1])))


def fit_model(gp, space, who: str) -> Model:
    """`gp.fit` on the real data, warnings silenced (theta search and its RandomState draws included), and its frame."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp.fit(space.params, space.target)
    return read_model(gp, space, who)


def pareto_gate(pareto, who: str, what: str):
    """The engine of a `ParetoOptimizer` whose models `who` can work on, else `ParetoOptimizer.suggest`'s refusals in its order:
    TargetSpaceEmptyError on an empty store; NotImplementedError for a device group (`what`: what a group lacks) and for an
    objective whose model would run on the host.  (suggest's fourth refusal, an observed front beyond gpbo_ehvi_argbest's level
    lists, belongs to that call alone.)"""
    from sklearn.base import clone

    if len(pareto) == 0:
        raise A.TargetSpaceEmptyError(A.EMPTY_SPACE_MESSAGE)
    eng = pareto._engine()
    if isinstance(eng, GroupEngine):
        raise NotImplementedError(f"{who}: a device group has no {what}; use a single device")
    for j, gp in enumerate(pareto._gps):
        reason = gp._unsupported_reason(clone(gp.kernel), pareto.targets[:, j], pareto.params)
        if reason is not None:
            raise NotImplementedError(f"{who}: objective {j}'s model runs on the host ({reason}); only models on the device path "
                                      "are served")
    return eng


#: the most draws a greedy draw batch takes: 16 groups of 16
MAX_DRAWS = MAX_QNEI_GROUPS * MAX_PATHS


def greedy_counts(q, n_random, n_draws, n_features):
    """(q, n_random, n_draws, n_features) as ints, else ValueError — the count checks of the greedy draw batches, in their order."""
    q = count(q, 1, MAX_SEEDS, f"q must be an integer in [1, {MAX_SEEDS}]")
    n_random, n_features = int(n_random), int(n_features)
    if n_random < 1:
        raise ValueError("n_random must be >= 1")
    if q > n_random:
        raise ValueError("q must not exceed n_random")
    n_draws = count(n_draws, 1, MAX_DRAWS, f"n_draws must be an integer in [1, {MAX_DRAWS}]")
    if not 1 <= n_features <= MAX_PATH_FEATURES:
        raise ValueError(f"n_features must be in [1, {MAX_PATH_FEATURES}]")
    return q, n_random, n_draws, n_features


def draw_layout(n_draws: int):
    """(G, S): `n_draws` as G = ceil(n_draws / 16) groups of S = ceil(n_draws / G) draws each — every group the same size, as the
    engine call wants them, so T = G * S >= n_draws (17 -> 2 x 9 = 18, 20 -> 2 x 10, 33 -> 3 x 11, 64 -> 4 x 16, 250 -> 16 x 16)."""
    G = -(-int(n_draws) // MAX_PATHS)
    return G, -(-int(n_draws) // G)


def pending_rows(pending, space, d: int):
    """`pending` (a list of parameter dicts, or an array (P, d)) as a float64 (P, d) array, None for no point"""
    if pending is None:
        return None
    if isinstance(pending, (list, tuple)) and len(pending) and all(isinstance(p, dict) for p in pending):
        try:
            pending = [[p[k] for k in space.keys] for p in pending]
        except KeyError as e:
            raise ValueError(f"pending: a point lacks the parameter {e.args[0]!r}") from None
    rows = np.asarray(pending, dtype=np.float64)
    if rows.size == 0:
        return None
    if rows.ndim != 2 or rows.shape[1] != d:
        raise ValueError(f"pending must be a list of parameter dicts or an array (P, {d})")
    if not np.isfinite(rows).all():
        raise ValueError("pending must be finite")
    return np.ascontiguousarray(rows)


def group_inputs(gp, rng, model, n_groups: int, n_paths: int, n_features: int):
    """`n_groups` groups of `n_paths` posterior draws as the greedy engine calls (`qnei_greedy`, `qnehvi_greedy`) take them: a list
    of (omega, phase, weights, eps), drawn from `rng` group after group in `draw_groups`' order — `spectral_draw` (fresh features),
    `standard_normal((S, F))`, `standard_normal((S, N))` scaled by sqrt(noise).  With a list of GPs and the list of their models
    (`cnei_greedy`'s slots): one such list per slot, drawn GROUP-MAJOR — per group, slot after slot."""
    from .thompson import spectral_draw

    several = isinstance(gp, (list, tuple))
    gps, models = (gp, model) if several else ([gp], [model])
    draws = [[] for _ in gps]
    for _ in range(n_groups):
        for groups, g, m in zip(draws, gps, models):
            omega, phase = spectral_draw(g._kind, n_features, m.d, rng)
            weights = rng.standard_normal((n_paths, n_features))
            groups.append((omega, phase, weights, rng.standard_normal((n_paths, m.N)) * np.sqrt(m.noise)))
    return draws if several else draws[0]


def picked_params(eng, index, d: int, to_params):
    """The tail of a greedy draw batch: (the picked candidate indices as int64, `to_params` of each picked row, fetched from the device)."""
    index = np.asarray(index, dtype=np.int64)
    rows = np.asarray(eng.get_candidate_rows(index, d), dtype=np.float64)
    return index, [to_params(x) for x in rows]


def draw_groups(gp, space, eng, rng, model: Model, n_draws: int, n_features: int, refine: int, max_iter, box=None):
    """`n_draws` posterior function draws over the resident candidates in groups of at most 16, one engine call per group: yields
    (first, S, result) with result what `ascend_paths(n_starts=refine)` returns, or with refine = 0 `sample_paths`.  Per group the
    draws from `rng`, in this order: `spectral_draw` (fresh features), `standard_normal((S, F))` — the feature weights —,
    `standard_normal((S, N))` scaled by sqrt(noise) — the noise draws.  The engine call draws nothing.  `box`: the (lo, hi) a climb
    stays inside (None: the space's bounds)."""
    from .thompson import spectral_draw

    box_lo, box_hi = (space.bounds[:, 0], space.bounds[:, 1]) if box is None else box
    for first in range(0, n_draws, MAX_PATHS):
        S = min(MAX_PATHS, n_draws - first)
        omega, phase = spectral_draw(gp._kind, n_features, model.d, rng)
        weights = rng.standard_normal((S, n_features))
        eps = rng.standard_normal((S, model.N)) * np.sqrt(model.noise)
        gp._ensure_resident()
        if refine:
            yield first, S, eng.ascend_paths(omega, phase, weights, eps, box_lo, box_hi, n_starts=refine,
                                             max_iter=-1 if max_iter is None else int(max_iter), slot=gp.slot,
                                             y_mean=model.y_mean, y_std=model.y_std)
        else:
            yield first, S, eng.sample_paths(omega, phase, weights, eps, slot=gp.slot, y_mean=model.y_mean, y_std=model.y_std)


def thompson_picks(gp, space, eng, rng, model: Model, q: int, n_features: int, refine: int, max_iter, box=None):
    """q parameter dicts, one per posterior draw over the resident candidates (`draw_groups`, its draws from `rng`): refine = 0 the
    draw's maximiser among the candidates, its row fetched from the device; refine = K the best of its K climbed runs inside `box`
    (None: the space's bounds) — a draw without a finite run keeps its first start, its best candidate."""
    picks = []
    for _first, n, out in draw_groups(gp, space, eng, rng, model, q, n_features, refine, max_iter, box):
        if refine:
            picks.extend(out["x_best"][s] if out["winner"][s] >= 0 else out["x"][s, 0] for s in range(n))
        else:
            picks.extend(int(i) for i in out[0])
    if refine:
        rows = np.asarray(picks, dtype=np.float64).reshape(q, model.d)
    else:
        rows = np.asarray(eng.get_candidate_rows(np.array(picks, dtype=np.int64), model.d), dtype=np.float64)
    return [space.array_to_params(x) for x in rows]
