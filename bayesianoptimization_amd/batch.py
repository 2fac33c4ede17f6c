"""suggest_batch(optimizer, q) — q points to probe in parallel from ONE candidate pass.

The reference's answer to "give me q points" is ConstantLiar (bayes_opt/acquisition.py:952-1178): every call registers the
earlier suggestions with a made-up target (the lie), refits the GP — theta search included — and runs a whole suggest().  Its q
calls cost q theta searches, q candidate draws and q posterior passes of N^2 work per candidate.

This module keeps the constant-liar idea and drops what the lie does not need to touch: theta and the targets' normalisation are
held at the real data's, and ONE candidate draw serves all q picks.  Then pick p + 1 differs from pick p by one appended row at
unchanged theta, which the engine takes as `fit_append` (O(N^2)) + `posterior_refresh` (one k* generation against the appended
row of W = L^-1, O(M N d)) + `acq_argbest` over the resident mu / sigma: one full posterior pass plus q - 1 cheap ones.
Not ConstantLiar's trajectory (it re-optimises theta on the lied-to data and redraws candidates), and not meant to be.
"""
from __future__ import annotations

import numpy as np

from . import _suggest as S
from . import fused_acquisition as A

_STOCK = (A.UpperConfidenceBound, A.ExpectedImprovement, A.ProbabilityOfImprovement, A.LogExpectedImprovement)


def _lie(strategy, target) -> float:
    """ConstantLiar.strategy (acquisition.py:1116-1128): 'min' / 'mean' / 'max' of the real targets, or a number."""
    if isinstance(strategy, (int, float, np.integer, np.floating)) and not isinstance(strategy, bool):
        return float(strategy)
    if strategy == "min":
        return float(target.min())
    if strategy == "mean":
        return float(target.mean())
    if strategy == "max":
        return float(target.max())
    raise ValueError(f"Received invalid argument {strategy} for strategy.")


def suggest_batch(optimizer, q: int, strategy="max", n_random: int | None = None):
    """q parameter dicts to probe side by side, as `optimizer.suggest()` returns one; `optimizer` has been `accelerate()`d.

    Constant liar at held theta and held target normalisation over one candidate draw:
      1. everything one `suggest(n_smart=0)` of the optimizer's policy does — its checks (TargetSpaceEmptyError on an empty space,
         ConstraintNotSupportedError with a constraint, as ConstantLiar), `gp.fit` with its theta search and RandomState draws, the
         candidates from the optimizer's RandomState on the device, the full posterior, the arg-best.  That is pick 1, bit for bit.
      2. for p = 2 .. q: the previous pick joins the slot's model with the lie as its target (`fit_append`; the lie is 'max' /
         'min' / 'mean' of the real targets or a float, normalised with the REAL data's mean and std), the resident posterior is
         refreshed (`posterior_refresh`) and the policy's arg-best is taken again, with y_max = max(real y_max, lie) for EI / POI / log EI.
      3. the policy's per-suggest bookkeeping advances once per pick — iteration counter, exploration decay — so that pick p uses
         the kappa / xi the p-th of q suggest() calls would have used.
      4. before returning, the estimator's incremental cache is dropped and the slot goes back to the fixed-theta fit of the real
         data: `gp.predict` answers for the real data, and the next `optimizer.suggest()` sees nothing of this call but the
         advanced RandomState and the policy's bookkeeping.
    Nothing keeps two picks apart but the lie: under 'max' a policy may pick one candidate twice, as ConstantLiar's can.
    A pick whose append crosses the slot's 64-row padding (N + p - 1 a multiple of 64) costs a full pass: the engine rebuilds there.
    `n_random`: candidates of the one draw (default: the policy's, the reference's 10_000).

    There is NO local-search stage in this version (the picks are the best of the random candidates): the device local search
    re-uses the candidate buffer the later picks still need.

    NotImplementedError, never a host fallback, for: a space with an input transform (int / categorical parameters), a policy
    other than stock UCB / EI / POI / log EI, a model in host mode (a kernel outside the device path), a device group.  q = 1 is valid;
    q < 1 is a ValueError."""
    q = S.count(q, 1, None, "q must be an integer >= 1", "q must be >= 1")
    fn = optimizer._acquisition_function
    if type(fn) not in _STOCK:
        raise NotImplementedError(f"suggest_batch: the policy is {type(fn).__name__}; only stock UpperConfidenceBound / "
                                  "ExpectedImprovement / ProbabilityOfImprovement / LogExpectedImprovement of an accelerate()d "
                                  "optimizer are batched")
    gp, space, eng = S.gate(optimizer, "suggest_batch", "batched", ("posterior_refresh",),
                            "a device group has no posterior refresh path; use a single device")
    lie = _lie(strategy, space.target)
    rng = optimizer._random_state

    # pick 1: the policy's own suggest(n_smart=0) — checks, fit, draw, full posterior, arg-best, bookkeeping
    picks = [np.asarray(fn.suggest(gp=gp, target_space=space, n_random=n_random, n_smart=0, fit_gp=True, random_state=rng),
                        dtype=np.float64)]
    model = S.read_model(gp, space, "suggest_batch")
    if q == 1:
        return [space.array_to_params(picks[0])]
    y_mean, y_std = model.y_mean, model.y_std
    y_real = np.asarray(gp.y_train_, dtype=np.float64).ravel()
    lie_norm = (lie - y_mean) / y_std
    extra = {} if model.scale is None else {"amplitude": model.scale[0], "white": model.scale[1]}
    improvement = isinstance(fn, A._ImprovementBased)
    if improvement:
        fn.y_max = max(float(fn.y_max), lie)       # the incumbent of a space that holds the lies (acquisition.py:1130-1143)
    try:
        gp._ensure_resident()
        for p in range(2, q + 1):
            y_norm = np.concatenate([y_real, np.full(p - 1, lie_norm)])
            gp._held = None                         # the slot is about to hold lies: no later fit may extend it
            eng.fit_append(gp._tx(picks[-1][None, :]), y_norm, slot=gp.slot, **extra)
            eng.posterior_refresh(gp.slot, y_mean, y_std, fetch=False)
            fn.i += 1
            best, _val, _seeds, _sv, _ys = eng.acq_argbest(fn._acq_kind, fn._acq_param(), fn.y_max if improvement else 0.0,
                                                           None, None, k_seeds=0)
            picks.append(np.asarray(eng.get_candidate_rows(np.array([int(best)]), model.d)[0], dtype=np.float64))
            fn.decay_exploration()
    finally:
        # the slot goes back to the real data at the held theta, whatever happened above
        gp._held = None
        gp._device_fit_tail()
    return [space.array_to_params(x) for x in picks]
