"""suggest_qnei(optimizer, q) — q points to probe in parallel by batch noisy expected improvement (qNEI; Letham, Karrer, Ottoni &
Bakshy 2019, "Constrained Bayesian optimization with noisy experiments"; the Monte-Carlo qEI of Wilson, Hutter & Deisenroth 2018).

Expected improvement needs an incumbent.  With observation noise the best MEASUREMENT (`space.target.max()`, what the EI policies
take) is itself noisy, and EI chases a lucky reading.  Here T joint draws f_t of the latent function are taken from the posterior
(the pathwise-conditioned draws of thompson.py), and each draw brings an incumbent of its own: its maximum over the points already
observed — and over points still pending.  A candidate is worth the mean over the draws of how far it lifts that incumbent,

    a(x) = 1/T sum_t max(f_t(x) - m_t, 0),

and a batch is built greedily: after a pick every draw's incumbent absorbs the draw's value there, m_t <- max(m_t, f_t(pick)), so
the next pick is scored JOINTLY with the earlier ones — no made-up observation as a constant liar needs (batch.py), no refit, and
unlike Thompson picks (thompson.py) not independently of each other.  The whole loop is ONE engine call (`qnei_greedy`,
gpbo_qnei_greedy; include/gpbo.h has the formulas and the conventions): the draws' values stay on the device as a (T, M) block, and
the q scoring passes, selections and incumbent updates run on the stream without a host round trip.
"""
from __future__ import annotations

import numpy as np

from . import _suggest as S
from ._lib import MAX_QNEI_POINTS as MAX_PENDING
from ._suggest import MAX_DRAWS, draw_layout  # noqa: F401  (their home is _suggest.py; they stay importable from here)


def suggest_qnei(optimizer, q: int, n_random: int = 10_000, n_draws: int = 64, n_features: int = 1024, noisy: bool = True,
                 pending=None, return_info: bool = False):
    """q parameter dicts to probe side by side, as `suggest_batch` returns them; `optimizer` has been `accelerate()`d.

      1. the checks of `suggest_thompson`, with its exception types (below).  The acquisition policy is neither consulted nor advanced.
      2. `gp.fit` on the real data, theta search (and its RandomState draws) included.
      3. ONE candidate draw of `n_random` points from the optimizer's RandomState, on the device.
      4. G = ceil(n_draws / 16) groups of S = ceil(n_draws / G) posterior draws: the engine call takes groups of one size, so
         T = G * S draws are taken, n_draws ROUNDED UP to a multiple of G (`draw_layout`; info["n_draws"] says how many).  Each
         group draws from the optimizer's RandomState in `suggest_thompson`'s order — `spectral_draw` (fresh features per group),
         `standard_normal((S, F))`, `standard_normal((S, N))` scaled by sqrt(noise) — one group after the other.
      5. ONE `qnei_greedy` call: the draws over the candidates, the incumbents, and the q greedy picks.  `noisy=True`: every draw's
         incumbent is its own maximum over the observed points; `noisy=False`: `space.target.max()` for every draw (plain
         Monte-Carlo qEI).  `pending` — a list of parameter dicts or an array (P, d), P <= 64: points suggested but not yet observed —
         is absorbed into every incumbent before the first pick.
      6. the picked rows are fetched from the device.
    No posterior pass, no local search: the picks are AMONG THE CANDIDATES.
    The zero-gain tail: once every draw's maximum among the candidates has been absorbed, no candidate lifts any incumbent and the
    best gain is exactly 0; the device's rule (ties to the lowest index) then hands out the lowest unpicked index.  The candidates are
    i.i.d. uniform, so that is a uniform random point of the space.  Such a pick is kept — the batch has q points, as asked — and
    reported: info["gain"] is 0 there.  With few draws this happens early (10 draws over 63 candidates: at the third pick).
    `return_info=True`: (picks, info) with info = {"gain": (q,) the gain of each pick when it was picked, "index": (q,) the picks'
    candidate indices, "baseline": (T,) the incumbents before the first pick, "n_draws": T}.
    Afterwards `gp.predict` answers for the real data as before; the slot holds the fit of step 2.

    ValueError: q not an integer in [1, 64] (or larger than `n_random`), n_random < 1, n_draws not an integer in [1, 256],
    n_features outside [1, 4096], more than 64 pending points, pending of another shape or not finite.  TargetSpaceEmptyError on an
    empty space, ConstraintNotSupportedError with a constraint.  NotImplementedError, never a host fallback, for: a GP that is not
    on the engine's slot 0, a space with an input transform (int / categorical parameters), a model in host mode, a device group."""
    q, n_random, n_draws, n_features = S.greedy_counts(q, n_random, n_draws, n_features)
    if pending is not None and len(pending) > MAX_PENDING:
        raise ValueError(f"pending must hold at most {MAX_PENDING} points")
    gp, space, eng = S.gate(optimizer, "suggest_qnei", "sampled", ("sample_paths", "qnei_greedy"),
                            "a device group has no path sampler; use a single device")
    pending = S.pending_rows(pending, space, int(space.bounds.shape[0]))
    rng = optimizer._random_state

    model = S.fit_model(gp, space, "suggest_qnei")
    eng.generate_candidates_like(n_random, space.bounds[:, 0], space.bounds[:, 1], rng)
    G, n_paths = draw_layout(n_draws)
    groups = S.group_inputs(gp, rng, model, G, n_paths, n_features)
    gp._ensure_resident()
    index, gain, baseline, _values, _keys = eng.qnei_greedy(groups, q, noisy=bool(noisy), y_best=float(np.max(space.target)),
                                                            pending=pending, slot=gp.slot, y_mean=model.y_mean, y_std=model.y_std)
    index, picks = S.picked_params(eng, index, model.d, space.array_to_params)
    if return_info:
        return picks, {"gain": np.asarray(gain, dtype=np.float64), "index": index, "baseline": np.asarray(baseline, dtype=np.float64),
                       "n_draws": G * n_paths}
    return picks
