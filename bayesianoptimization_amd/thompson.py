"""suggest_thompson(optimizer, q) — q points to probe in parallel by Thompson sampling: q function draws from the GP posterior over
ONE candidate set, each draw's maximiser a pick.

The other standard way to a batch besides a constant liar (batch.py): no lie, no incumbent, no acquisition formula — the posterior's
own spread keeps the picks apart.  scikit-learn's route to a posterior draw is GaussianProcessRegressor.sample_y (_gpr.py):
predict(return_cov=True), an M x M covariance and its factorisation on the host, which ends at a few thousand candidates.  Here a
draw is conditioned pathwise (Matheron's rule; Wilson et al. 2020, "Efficiently sampling functions from Gaussian process
posteriors"): a random-Fourier-feature draw from the prior plus an exact data-dependent update, evaluated by the engine's
`sample_paths` (gpbo_sample_paths) at O((N + F) d) per candidate for 16 draws at once.  Only the prior part is approximate, through
the F features; include/gpbo.h has the formulas.  A draw is a closed-form function, so with `refine=K` each one is also CLIMBED from
its K best candidates to a local maximiser inside the bounds (the engine's `ascend_paths`, gpbo_ascend_paths: value and gradient
at O((N + F) d) per evaluation, optimiser and evaluations in one launch) — the local-search stage of the reference's suggest().
"""
from __future__ import annotations

import numpy as np

from . import _suggest as S
# features per draw, starts per draw one ascend_paths call climbs from (draws per call: _suggest.draw_groups)
from ._lib import MAX_PATH_FEATURES as MAX_FEATURES, MAX_PATH_STARTS as MAX_STARTS

#: the kernel kinds of include/gpbo.h -> Matern nu (RBF: the Gaussian spectrum)
_NU = {1: 2.5, 2: 1.5, 3: 0.5}


def spectral_draw(kind: int, n_features: int, d: int, random_state):
    """(omega (F, d), phase (F,)) of F random Fourier features of a unit-length-scale kernel of `kind` (0 RBF, 1 / 2 / 3 Matern
    nu = 2.5 / 1.5 / 0.5) in d dimensions, in the units gpbo_sample_paths takes: omega in TURNS per unit of the length-scaled input
    (the angular frequency / 2 pi), phase in turns, so that  2 / F  sum_j cos(2 pi (omega_j . a + phase_j)) cos(2 pi (omega_j . b +
    phase_j))  estimates k(a, b) for length-scaled a, b.

    Angular frequencies from the kernel's spectral density: RBF w = z, z ~ N(0, I); Matern nu: w = z / sqrt(u / (2 nu)), u ~
    chi^2(2 nu), one u per feature (a multivariate t with 2 nu degrees of freedom; nu = 0.5 is Cauchy-tailed).

    The draws from `random_state` (a numpy RandomState), in this fixed order:
        standard_normal((F, d));  chisquare(2 nu, F) — Matern only;  uniform(size=F)."""
    kind, F, d = int(kind), int(n_features), int(d)
    if kind != 0 and kind not in _NU:
        raise ValueError(f"spectral_draw: unknown kernel kind {kind}")
    if F < 1 or d < 1:
        raise ValueError("spectral_draw: n_features and d must be >= 1")
    w = random_state.standard_normal((F, d))
    if kind != 0:
        nu2 = 2.0 * _NU[kind]
        u = random_state.chisquare(nu2, F)
        w = w / np.sqrt(u / nu2)[:, None]
    phase = random_state.uniform(size=F)
    return np.ascontiguousarray(w / (2.0 * np.pi)), phase


def suggest_thompson(optimizer, q: int, n_random: int = 10_000, n_features: int = 1024, refine: int = 0, max_iter=None):
    """q parameter dicts to probe side by side, as `suggest_batch` returns them; `optimizer` has been `accelerate()`d.

      1. the checks of `suggest_batch`, with its exception types (below).  The acquisition policy is neither consulted nor advanced.
      2. `gp.fit` on the real data, theta search (and its RandomState draws) included.
      3. ONE candidate draw of `n_random` points from the optimizer's RandomState, on the device.
      4. ceil(q / 16) `sample_paths` calls of up to 16 draws.  Each call draws from the optimizer's RandomState, in this order:
         `spectral_draw` (fresh features per call), `standard_normal((S, F))` — the feature weights — and `standard_normal((S, N))`
         scaled by sqrt(noise) — the noise draws, noise = the estimator's alpha (+ the WhiteKernel's level for a scaled model).
      5. the picked rows are fetched from the device.
    No posterior pass.  With `refine=0` (the default) there is no local search either: the picks are the draws' maximisers AMONG THE
    CANDIDATES.  Two draws may pick the same candidate (a sharply peaked posterior: every draw agrees); that is kept — the caller sees
    how decided the model is.
    `refine=K`, 1 <= K <= 8: each group of up to 16 draws is ONE `ascend_paths` call in place of its `sample_paths` call (steps 4 and
    5; no candidate rows are fetched): every draw is climbed from its K best candidates to a local maximiser inside `space.bounds` on
    the device, and the pick is the best of its K runs.  The optimiser accepts no worse point, so a pick's value under its draw is at
    least its best candidate's.  The refinement draws nothing: the optimizer's RandomState ends where `refine=0` leaves it.
    `max_iter` (None: 15 000) bounds the iterations of a run.
    `n_features` = 1024: at 256 the variance of the draws is already off by 25 % for Matern nu = 1.5 / 2.5 (tests/test_thompson_host.py).
    Afterwards `gp.predict` answers for the real data as before; the slot holds the fit of step 2.

    ValueError: q not an integer >= 1, n_random < 1, n_features outside [1, 4096], refine not an integer in [0, 8] (or larger than
    `n_random`: a draw has no more starts than candidates).  TargetSpaceEmptyError on an empty space,
    ConstraintNotSupportedError with a constraint.  NotImplementedError, never a host fallback, for: a GP that is not on the engine's
    slot 0, a space with an input transform (int / categorical parameters), a model in host mode, a device group."""
    q = S.count(q, 1, None, "q must be an integer >= 1", "q must be >= 1")
    n_random, n_features = int(n_random), int(n_features)
    if n_random < 1:
        raise ValueError("n_random must be >= 1")
    if not 1 <= n_features <= MAX_FEATURES:
        raise ValueError(f"n_features must be in [1, {MAX_FEATURES}]")
    gp, space, eng = S.gate(optimizer, "suggest_thompson", "sampled", ("sample_paths",),
                            "a device group has no path sampler; use a single device")
    refine = S.count(refine, 0, MAX_STARTS, f"refine must be an integer in [0, {MAX_STARTS}]")
    if refine and not hasattr(eng, "ascend_paths"):
        raise NotImplementedError("suggest_thompson: the engine has no ascend_paths")
    rng = optimizer._random_state

    model = S.fit_model(gp, space, "suggest_thompson")
    eng.generate_candidates_like(n_random, space.bounds[:, 0], space.bounds[:, 1], rng)
    return S.thompson_picks(gp, space, eng, rng, model, q, n_features, refine, max_iter)
