"""A 50-digit truth (mpmath) for the log constrained expected improvement and the log feasibility (GPBO_ACQ_LOG_CEI = 5,
GPBO_ACQ_LOG_FEAS = 6), on tests/log_ei_truth.py's pattern, and a NumPy / SciPy restatement of the header's words for c_ref.

Every site (acq_value, gpbo_polish_seeds' host side, LogConstrainedExpectedImprovement's host objective) starts from fp64 posteriors
and forms `aa = mu - y_max - xi`, `a_j = (lb_j - cm) / cs`, `b_j = (ub_j - cm) / cs` in fp64, so the truth takes THOSE fp64 values as
given and is exact from there on:

    log p_j = log(Phi(b_j) - Phi(a_j))   (an infinite bound: Phi = 0 / 1; an interval in the upper tail is evaluated reflected)
    key     = -(logEI + sum_j log p_j)   kind 5;   -(sum_j log p_j)   kind 6
    gradient of the key:  -(ca dmu + cs dsd) - sum_j dlog p_j,
                          dlog p_j = (q_b (-dcm - b dcs) - q_a (-dcm - a dcs)) / cs_j,  q_x = phi(x) / p_j

(The working precision is raised by the squared magnitude of the finite bounds, as log_ei_truth raises it for z, and by the digits
the subtraction Phi(b) - Phi(a) of a narrow band cancels.)

Error model, derived, not measured: |value - truth| <= c eps W,

    W = 1 + z^2 + |logEI| + sum_j (1 + kappa_j + |log p_j|),   kappa_j = (|a_j| phi(a_j) + |b_j| phi(b_j)) / p_j over the finite bounds

kappa_j is the condition number of log p_j against half an ulp in the divisions that make a_j and b_j (d log p / db = phi(b) / p, and
the division leaves b with an error of |b| eps / 2) — for ANY implementation; in a one-sided lower tail it is the b^2 that z^2 is for
logEI.  The sum rounds at the scale of its terms, hence the |log p_j| and the 1 per term.  Kind 6 drops the logEI terms.
Gradient, per component: a term t_x = q_x (-dcm - x dcs) / cs carries the relative error of q_x = exp(-x^2/2 - log(2 pi)/2 - log p_j)
— the exponent's absolute error: x^2 eps from the rounding of x^2 / 2 and of x itself, the error of log p_j, (1 + kappa_j + |log p_j|) eps,
and the subtraction's — and the rounding of the inner sum at the scale of its terms:

    W_g = (1 + z^2)(|ca dmu| + |cs dsd|) + sum_j sum_{x in finite bounds} (1 + x^2 + kappa_j + |log p_j|) q_x (|dcm| + |x dcs|) / cs_j

which is log_ei_truth's w_g with the constraint terms' own factor.  Where a q_x lies below the normal numbers (a bound 39 sigma or
more inside the band's far side: phi(x) / p_j < DBL_MIN) fp64 holds no relative error any more: the gradient's bar carries acq_truth's
floor, DBL_MIN per such term at the scale of its factor, `floor_g` = sum DBL_MIN (|dcm| + |x dcs|) / cs_j.
`acq_truth.constants(got, truth, W, floor=0.0)` gives c for the values, `constants(got, truth, W, floor_g)` here for the gradient."""
import numpy as np

import acq_truth as T
import log_ei_truth as L

_ctx = T._ctx
_NAN = T._NAN
LOG_CEI, LOG_FEAS = 5, 6


def _digits(a, b):
    """working digits for one band: 50 are left after the squared magnitude of the finite bounds (as log_ei_truth's for z) and after
    the digits the subtraction Phi(b) - Phi(a) of a narrow band cancels (its width against the nearer bound's Mills ratio ~ 1 / |x|)"""
    fin = [abs(float(x)) for x in (a, b) if np.isfinite(x)]
    big = max(fin + [1.0])
    lost = 0
    if len(fin) == 2:
        share = min(1.0, abs(float(b) - float(a)) * (1.0 + min(fin)))
        lost = int(np.ceil(-np.log10(max(share, 1e-300))))
    return T.DPS + 10 + lost + 2 * int(np.ceil(np.log10(big)))


_WORKING = {}


def _working(dps):
    """an mpmath context of `dps` digits (made once per precision: a clone costs as much as the band it serves)"""
    if dps not in _WORKING:
        _WORKING[dps] = _ctx.clone()
        _WORKING[dps].dps = dps
    return _WORKING[dps]


def band_log_truth(a, b):
    """One band from its fp64 standardised bounds a < b (either may be infinite): (log p, kappa, q_a, q_b) as 50-digit mpf, q_x =
    phi(x) / p (0 for an infinite bound).  An interval in the upper tail is evaluated reflected."""
    work = _working(_digits(a, b))
    fa, fb = np.isfinite(a), np.isfinite(b)
    if not fa and not fb:
        zero = _ctx.mpf(0)
        return zero, zero, zero, zero
    flip = fa and a >= 0
    lo, hi = (-b, -a) if flip else (a, b)                      # Phi(hi) - Phi(lo) is the same number
    sqrt2 = work.sqrt(2)

    def Phi(x):
        if not np.isfinite(x):
            return work.mpf(1 if x > 0 else 0)
        return work.erfc(-work.mpf(float(x)) / sqrt2) / 2

    def phi(x):
        x = work.mpf(float(x))
        return work.exp(-x * x / 2) / work.sqrt(2 * work.pi)

    p = Phi(hi) - Phi(lo)
    log_p = work.log(p)
    pa = phi(a) if fa else work.mpf(0)
    pb = phi(b) if fb else work.mpf(0)
    kappa = ((abs(work.mpf(float(a))) * pa if fa else 0) + (abs(work.mpf(float(b))) * pb if fb else 0)) / p
    return _ctx.mpf(log_p), _ctx.mpf(kappa), _ctx.mpf(pa / p), _ctx.mpf(pb / p)


def standardise(lb, ub, cm, cs):
    """the fp64 a, b every site forms (-inf / +inf for an infinite bound, without a division)"""
    cm, cs = np.asarray(cm, dtype=np.float64), np.asarray(cs, dtype=np.float64)
    with np.errstate(all="ignore"):
        a = (lb - cm) / cs if lb != -np.inf else np.full(cm.shape, -np.inf)
        b = (ub - cm) / cs if ub != np.inf else np.full(cm.shape, np.inf)
    return a, b


def log_cei_truth(kind, mu, sd, y_max, xi, cons, dmu=None, dsd=None, dcons=None, ei=None):
    """Truth for n points.  `cons`: [(lb, ub, cm (n,), cs (n,))] per constraint; with dmu, dsd (n, d) and `dcons` [(dcm, dcs)] per
    constraint also the gradient; `ei`: log_ei_truth's answer for the same mu, sd, y_max, xi (and dmu, dsd), where the caller holds
    it already.  Returns a dict: `ok` (the truth is defined: finite inputs, cs > 0, a < b — and for kind 5 sd > 0),
    `key` (mpf, the selection key), `w` (mpf), `key_feas` / `w_feas` (kind 6's key and weight, whatever `kind` is), `log_p` [(n,) mpf per constraint], `kappa` likewise, and `g`, `w_g` (n, d)."""
    n = np.shape(cons[0][2] if cons else mu)[0]
    with_ei = kind == LOG_CEI
    ok = np.ones(n, dtype=bool)
    if with_ei:
        ei = L.log_ei_truth(mu, sd, y_max, xi, dmu, dsd) if ei is None else ei
        ok &= ei["ok"]
    ab = []
    for lb, ub, cm, cs in cons:
        cm, cs = np.asarray(cm, dtype=np.float64), np.asarray(cs, dtype=np.float64)
        a, b = standardise(lb, ub, cm, cs)
        ab.append((a, b))
        ok &= np.isfinite(cm) & np.isfinite(cs) & (cs > 0) & (a < b)
    key, w, key_feas, w_feas = ([_NAN] * n for _ in range(4))
    log_p = [[_NAN] * n for _ in cons]
    kappa = [[_NAN] * n for _ in cons]
    d = None if dmu is None and dcons is None else np.asarray(dcons[0][0] if dcons else dmu).reshape(n, -1).shape[1]
    g = wg = None
    if d is not None:
        g, wg = np.full((n, d), _NAN, dtype=object), np.full((n, d), _NAN, dtype=object)
        floor_g = np.zeros((n, d))
    for i in np.flatnonzero(ok):
        total = ei["log_ei"][i] if with_ei else _ctx.mpf(0)
        weight = ei["w"][i] if with_ei else _ctx.mpf(0)
        feas, feas_weight = _ctx.mpf(0), _ctx.mpf(0)
        gi = [ei["g"][i, k] if with_ei else _ctx.mpf(0) for k in range(d or 0)]
        wgi = [ei["w_g"][i, k] if with_ei else _ctx.mpf(0) for k in range(d or 0)]
        for j, (lb, ub, cm, cs) in enumerate(cons):
            a, b = float(ab[j][0][i]), float(ab[j][1][i])
            lp, kap, qa, qb = band_log_truth(a, b)
            log_p[j][i], kappa[j][i] = lp, kap
            total += lp
            feas += lp
            weight += 1 + kap + abs(lp)
            feas_weight += 1 + kap + abs(lp)
            if d is None:
                continue
            s = _ctx.mpf(float(np.asarray(cs)[i]))
            dcm, dcs = (np.asarray(v, dtype=np.float64).reshape(n, -1) for v in dcons[j])
            for k in range(d):
                slope, wk = _ctx.mpf(0), _ctx.mpf(0)
                for x, q, sign in ((b, qb, 1), (a, qa, -1)):
                    if not np.isfinite(x):
                        continue
                    xm, m1, s1 = _ctx.mpf(x), _ctx.mpf(float(dcm[i, k])), _ctx.mpf(float(dcs[i, k]))
                    slope += sign * q * (-m1 - xm * s1) / s
                    wk += (1 + xm * xm + kap + abs(lp)) * q * (abs(m1) + abs(xm * s1)) / s
                    floor_g[i, k] += float(T.DBL_MIN * (abs(m1) + abs(xm * s1)) / s)
                gi[k] -= slope
                wgi[k] += wk
        key[i], w[i], key_feas[i], w_feas[i] = -total, weight, -feas, feas_weight
        if d is not None:
            g[i, :], wg[i, :] = gi, wgi
    out = {"ok": ok, "key": T._obj(key), "w": T._obj(w), "log_p": [T._obj(v) for v in log_p], "kappa": [T._obj(v) for v in kappa],
           "ab": ab, "key_feas": T._obj(key_feas), "w_feas": T._obj(w_feas)}
    if d is not None:
        out["g"], out["w_g"], out["floor_g"] = g, wg, floor_g
    return out


def constants(got, truth, weight, floor):
    """acq_truth.constants with a floor per element"""
    got = np.asarray(got, dtype=np.float64)
    floor = np.broadcast_to(np.asarray(floor, dtype=np.float64), got.shape)
    out = np.empty(got.size)
    for i, (g, t, w, f) in enumerate(zip(np.ravel(got), np.ravel(truth), np.ravel(weight), np.ravel(floor))):
        out[i] = T.constants(np.array([g]), [t], [w], floor=float(f))[0]
    return out.reshape(got.shape)


# ---- the formula in NumPy / SciPy, written from its definition (include/gpbo.h), for c_ref ----------------------------------------
def _log_ndtr(x):
    from scipy.special import erfcx, ndtr

    if np.isnan(x):
        return np.nan
    if x > -1.0:
        return np.log(ndtr(x))
    return -(x * x) / 2.0 + np.log(erfcx(-x / np.sqrt(2.0))) - np.log(2.0)


def _log_p(lb, ub, cm, cs):
    """(log p_j, a, b) at one point"""
    from scipy.special import erf

    lb, ub, cm, cs = np.float64(lb), np.float64(ub), np.float64(cm), np.float64(cs)
    a = (lb - cm) / cs if lb != -np.inf else -np.inf
    b = (ub - cm) / cs if ub != np.inf else np.inf
    if lb == -np.inf and ub == np.inf:
        return 0.0, a, b
    if not cs > 0.0:
        return np.nan, a, b
    if lb == -np.inf:
        return _log_ndtr(b), a, b
    if ub == np.inf:
        return _log_ndtr(-a), a, b
    if np.isnan(a) or np.isnan(b) or a > b:
        return np.nan, a, b
    if a == b:
        return -np.inf, a, b
    lo, hi = (-b, -a) if a >= 0.0 else (a, b)
    r = 1.0 / np.sqrt(2.0)
    if hi <= 0.0:
        if lo > -1.0:
            return np.log(0.5 * (erf(hi * r) - erf(lo * r))), a, b
        lph, lpl = _log_ndtr(hi), _log_ndtr(lo)
        return lph + np.log(-np.expm1(lpl - lph)), a, b
    return np.log(0.5 * (erf(hi * r) + erf(-lo * r))), a, b


def reference_values(kind, mu, sd, y_max, xi, cons, dmu=None, dsd=None, dcons=None):
    """The selection key (n,) — and with the posteriors' input gradients its gradient (n, d) — point by point in fp64: the recipe as
    the header words it, not the policy's code.  Kind 5 without a constraint is log_ei_truth's restatement, negated."""
    n = np.shape(cons[0][2] if cons else mu)[0]
    with_grad = dmu is not None or dcons is not None
    d = np.asarray(dcons[0][0] if dcons else dmu).reshape(n, -1).shape[1] if with_grad else 0
    with np.errstate(all="ignore"):
        if kind == LOG_CEI:
            got = L.reference_values(mu, sd, y_max, xi, dmu, dsd) if with_grad else (L.reference_values(mu, sd, y_max, xi), None)
            total, g = got[0].copy(), (got[1].copy() if with_grad else None)
        else:
            total, g = np.zeros(n), (np.zeros((n, d)) if with_grad else None)
        for j, (lb, ub, cm, cs) in enumerate(cons):
            cm, cs = np.asarray(cm, dtype=np.float64), np.asarray(cs, dtype=np.float64)
            for i in range(n):
                lp, a, b = _log_p(lb, ub, cm[i], cs[i])
                total[i] = total[i] + lp
                if not with_grad:
                    continue
                dcm, dcs = (np.asarray(v, dtype=np.float64).reshape(n, -1) for v in dcons[j])
                qa = 0.0 if np.isinf(a) else np.exp(-(a * a) / 2.0 - 0.5 * np.log(2.0 * np.pi) - lp)
                qb = 0.0 if np.isinf(b) else np.exp(-(b * b) / 2.0 - 0.5 * np.log(2.0 * np.pi) - lp)
                for k in range(d):
                    tb = 0.0 if np.isinf(b) else qb * (-dcm[i, k] - b * dcs[i, k])
                    ta = 0.0 if np.isinf(a) else qa * (-dcm[i, k] - a * dcs[i, k])
                    g[i, k] = g[i, k] - (tb - ta) / cs[i]
        key = -1.0 * total
    return (key, g) if with_grad else key


def reference_product(mu, sd, y_max, xi, cons):
    """The reference's constrained EI in NumPy, as acquisition.py and constraint.py form it: -1 * EI * prod_j (cdf(ub) - cdf(lb))."""
    ei = T.reference_values(np.asarray(mu), np.asarray(sd), y_max, xi)[0]
    p = None
    for lb, ub, cm, cs in cons:
        pj = T.reference_band(np.asarray(cm), np.asarray(cs), lb, ub)
        p = pj if p is None else p * pj
    return -1 * ei * p


def argbest(keys):
    """the truth's order of the keys (mpf; ties to the lowest index)"""
    return sorted(range(len(keys)), key=lambda i: (keys[i], i))


# ---- the small constrained problem of the GPU tests (tests/test_gpu_log_cei.py) and of the host test of their condition ------------
SMALL_N, SMALL_D, SMALL_M, SMALL_LS, SMALL_NOISE = 24, 2, 2000, 0.3, 1e-6
#: the case in which the constrained product is a plateau of zeros: the band lies 7 sigma or more above every candidate's constraint
#: posterior (means in [-1.0, 0.9], deviations up to 0.45), where Phi(b) - Phi(a) is 1 - 1
PLATEAU_LB, PLATEAU_UB = 4.0, 4.5


def small_problem(M=SMALL_M):
    """(X (24, 2), y, c1, c2, Xc (M, 2)): a target and two constraint functions on the unit square, fitted at fixed theta (Matern 2.5,
    length scale 0.3, noise 1e-6) by the tests"""
    rng = np.random.RandomState(24)
    X = rng.uniform(size=(SMALL_N, SMALL_D))
    y = np.sin(3.0 * X.sum(1)) + 0.5 * X[:, 0]
    c1 = np.cos(2.0 * X.sum(1))
    c2 = X[:, 0] - X[:, 1]
    Xc = np.random.RandomState(5).uniform(size=(M, SMALL_D))
    return X, y, c1, c2, Xc
