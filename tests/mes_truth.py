"""Truth for max-value entropy search (tests only; never imported by the product).

    gamma_s(x) = (y*_s - mu(x)) / sd(x)
    a(x)       = 1/S sum_s h(gamma_s(x)),      h(g) = g phi(g) / (2 Phi(g)) - log Phi(g)

`h_truth`: h in mpmath at 60 digits with Phi taken from erfc on BOTH sides and -log Phi through the complement for g > 0 (at 50
digits log(Phi(g)) of a Phi formed directly is already rounded at g > 14 and the "truth" is off by 1 %).  60 digits carry the
cancellation of the two halves down to g = -1e6 (each half ~ g^2 / 2 = 5e11, the difference ~ log|g|).
`mes_values`: the three-range form of include/gpbo.h in NumPy / SciPy, with the conventions (sd == 0 -> 0, NaN propagates); held to
`h_truth` in tests/test_mes_host.py.
`argbest`: numpy's argmin / min / stable argsort[:k] over a key, as gpbo_acq_argbest states them.
"""
import mpmath
import numpy as np
from scipy import special

_ctx = mpmath.mp.clone()
_ctx.dps = 60

BAR = 1e-9             # the project's bar on a MES value, relative ...
TINY = 1e-290          # ... with values below this held to BAR * TINY absolutely (h is subnormal above gamma ~ 37)
SERIES_BELOW = -28.0   # csrc/acq_formulas.h: LOG_EI_SERIES_BELOW
HALF_LOG_2PI = 0.91893853320467274178


def h_truth(g):
    """h(g) as an mpmath number (60 digits); g a float (exactly representable values are taken exactly)"""
    c = _ctx
    g = c.mpf(g)
    phi = c.exp(-g * g / 2) / c.sqrt(2 * c.pi)
    if g > 0:
        q = c.erfc(g / c.sqrt(2)) / 2
        return g * phi / (2 * (1 - q)) - c.log1p(-q)
    cdf = c.erfc(-g / c.sqrt(2)) / 2
    return g * phi / (2 * cdf) - c.log(cdf)


def h_truth_f(g):
    return float(h_truth(g))


def gamma_mp(y, mu, sd):
    """(y - mu) / sd of three floats, formed in 60 digits"""
    return (_ctx.mpf(float(y)) - _ctx.mpf(float(mu))) / _ctx.mpf(float(sd))


def _ratio(g):
    """r = 1 + g Phi(g) / phi(g) for g <= -1: erfcx down to SERIES_BELOW, ten terms of the asymptotic series below it"""
    g = np.asarray(g, dtype=np.float64)
    r = np.empty_like(g)
    near = g > SERIES_BELOW
    t = -g[near] * 0.70710678118654752440
    r[near] = 1.0 - 1.77245385090551602730 * t * special.erfcx(t)
    w = 1.0 / (g[~near] * g[~near])
    s = np.full_like(w, -654729075.0)
    for c in (34459425.0, -2027025.0, 135135.0, -10395.0, 945.0, -105.0, 15.0, -3.0, 1.0):
        s = s * w + c
    r[~near] = w * s
    return r


def h_values(g):
    """h over an array of gammas by the three-range form (NaN -> NaN, 0 from gamma = 40 on, the limit form below -1e150)"""
    g = np.asarray(g, dtype=np.float64)
    out = np.full(g.shape, np.nan)
    with np.errstate(all="ignore"):
        up = g > 0.0
        gu = np.minimum(g[up], 40.0)
        q = 0.5 * special.erfc(gu * 0.70710678118654752440)
        out[up] = gu * (np.exp(-(gu * gu) / 2.0) / 2.50662827463100050242) / (2.0 * (1.0 - q)) - np.log1p(-q)
        mid = (g <= 0.0) & (g > -1.0)
        gm = g[mid]
        cdf = special.ndtr(gm)
        out[mid] = gm * (np.exp(-(gm * gm) / 2.0) / 2.50662827463100050242) / (2.0 * cdf) - np.log(cdf)
        far = g < -1e150
        out[far] = -0.5 + HALF_LOG_2PI + np.log(-g[far])
        low = (g <= -1.0) & ~far
        gl = g[low]
        r = _ratio(gl)
        m = (1.0 - r) / (-gl)
        out[low] = gl * r / (2.0 * m) + HALF_LOG_2PI - np.log(m)
    return out


def mes_values(mu, sd, y_star):
    """a(x) (M,) >= 0 from mu, sd (M,) and the sampled maxima y_star (S,): the sum over s in the order s = 0 .. S - 1, then one
    division by S.  sd == 0 -> 0 unless mu is NaN; a NaN mu or sd -> NaN."""
    mu, sd = np.asarray(mu, dtype=np.float64), np.asarray(sd, dtype=np.float64)
    y_star = np.atleast_1d(np.asarray(y_star, dtype=np.float64))
    acc = np.zeros(mu.shape)
    with np.errstate(all="ignore"):
        for y in y_star:
            acc = acc + h_values((y - mu) / sd)
    a = acc / float(y_star.shape[0])
    a = np.where((sd == 0.0) & ~np.isnan(mu), 0.0, a)
    return np.where(np.isnan(mu) | np.isnan(sd), np.nan, a)


def within_bar(got, want, bar=BAR):
    """(worst |got - want| / max(|want|, TINY), ok) elementwise over finite `want`; NaNs must sit at the same places"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return np.inf, False
    fin = ~np.isnan(want)
    same_inf = np.isinf(want[fin]) & (got[fin] == want[fin])
    with np.errstate(all="ignore"):
        err = np.where(same_inf, 0.0, np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), TINY))
    worst = float(err.max()) if err.size else 0.0
    return worst, worst <= bar


def argbest(ys, k=0, index_offset=0):
    """(best_idx, best_val, seed_idx (k,), seed_val (k,)) of the key ys: argmin / min with the first NaN winning; argsort[:k] with
    ties to the lowest index, -0.0 == 0.0 and NaNs last"""
    ys = np.asarray(ys, dtype=np.float64)
    nan = np.isnan(ys)
    if nan.any():
        bi, bv = int(np.flatnonzero(nan)[0]), float("nan")
    else:
        bi, bv = int(ys.argmin()), float(ys.min())
    order = np.lexsort((np.arange(len(ys)), np.where(nan, np.inf, ys) + 0.0, nan))[:k]
    return bi + index_offset, bv, order + index_offset, ys[order]


def separated_top(a, k, bar=BAR):
    """True when no two of the k + 1 largest a (ties in rank included) lie within `bar` relative of each other: the ranking of the
    top k is then the same for every evaluation within the bar"""
    a = np.asarray(a, dtype=np.float64)
    top = np.sort(a[~np.isnan(a)])[::-1][:k + 1]
    if top.size < 2:
        return True
    return bool(np.all(top[:-1] - top[1:] > 2.0 * bar * np.maximum(np.abs(top[:-1]), TINY)))
