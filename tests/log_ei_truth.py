"""A 50-digit truth (mpmath) for log expected improvement, on tests/acq_truth.py's context and conventions, and a NumPy restatement
of the formula for c_ref.

Every site (acq_value, polish_acq_coeffs on the device and on the host, LogExpectedImprovement.base_acq) starts from fp64 mu, sd and
forms `aa = mu - y_max - xi` left to right in fp64, so the truth takes THAT fp64 aa as given and is exact from there on:

    z = aa / sd,  h(z) = phi(z) + z Phi(z),  logEI = log(sd) + log h(z)
    gradient of -logEI:  g = -(ca dmu + cs dsd),  ca = Phi / (sd h),  cs = phi / (sd h)

(h cancels z^2-fold in the lower tail: the working precision is raised by 2 log10|z| + 20 digits so that 50 are left.)

Error model: |value - truth| <= c eps W,  W = 1 + z^2 + |truth|: half an ulp in the division that makes z moves log h by ~ z^2 eps in
the lower tail (d log h / dz ~ -z) for ANY implementation, the sum log(sd) + log h rounds at the scale of its terms — which is the
scale of the result except where they cancel, hence the 1 —; gradient: W_g = (1 + z^2)(|ca dmu| + |cs dsd|), as acq_truth's.
`acq_truth.constants(got, truth, W)` gives c per element."""
import numpy as np

import acq_truth as T

_ctx = T._ctx
_NAN = T._NAN


def log_ei_truth(mu, sd, y_max, xi, dmu=None, dsd=None):
    """Truth for fp64 mu, sd (n,).  Returns a dict: `ok` (finite aa, sd and sd > 0: the truth is defined), `z` (fp64), `log_ei` (mpf; the
    ACQUISITION, not its negative), `w` (mpf weight W); with dmu, dsd (n, d) also `g` (mpf, the gradient of -logEI) and `w_g`."""
    mu = np.asarray(mu, dtype=np.float64)
    sd = np.asarray(sd, dtype=np.float64)
    n = mu.shape[0]
    aa = mu - y_max - xi                                    # the fp64 value every site forms
    ok = np.isfinite(aa) & np.isfinite(sd) & (sd > 0)
    val, w, ca_, cs_, zs = ([_NAN] * n for _ in range(5))
    for i in np.flatnonzero(ok):
        work = _ctx.clone()
        zf = abs(float(aa[i]) / float(sd[i]))
        work.dps = T.DPS + 20 + (2 * int(np.ceil(np.log10(zf))) if zf > 1 and np.isfinite(zf) else 0)
        a, s = work.mpf(float(aa[i])), work.mpf(float(sd[i]))
        z = a / s
        P = work.erfc(-z / work.sqrt(2)) / 2
        p = work.exp(-z * z / 2) / work.sqrt(2 * work.pi)
        h = p + z * P
        v = work.log(s) + work.log(h)
        zs[i], val[i], w[i] = _ctx.mpf(z), _ctx.mpf(v), _ctx.mpf(1 + z * z + abs(v))
        ca_[i], cs_[i] = _ctx.mpf(P / (s * h)), _ctx.mpf(p / (s * h))
    out = {"ok": ok, "log_ei": T._obj(val), "w": T._obj(w)}
    with np.errstate(all="ignore"):
        out["z"] = np.where(ok, aa / sd, np.nan)
    if dmu is not None:
        dmu = np.asarray(dmu, dtype=np.float64).reshape(n, -1)
        dsd = np.asarray(dsd, dtype=np.float64).reshape(n, -1)
        d = dmu.shape[1]
        g = np.full((n, d), _NAN, dtype=object)
        wg = np.full((n, d), _NAN, dtype=object)
        for i in np.flatnonzero(ok & np.all(np.isfinite(dmu), axis=1) & np.all(np.isfinite(dsd), axis=1)):
            for j in range(d):
                tm, ts = ca_[i] * _ctx.mpf(float(dmu[i, j])), cs_[i] * _ctx.mpf(float(dsd[i, j]))
                g[i, j] = -(tm + ts)
                wg[i, j] = (1 + zs[i] * zs[i]) * (abs(tm) + abs(ts))
        out["g"], out["w_g"] = g, wg
    return out


# ---- the formula in NumPy / SciPy, written from its definition (include/gpbo.h), for c_ref ----------------------------------------
SERIES_BELOW = -28.0
DOUBLE_FACTORIALS = [1.0, 3.0, 15.0, 105.0, 945.0, 10395.0, 135135.0, 2027025.0, 34459425.0, 654729075.0]   # (2k + 1)!!, k = 0 ... 9


def _ratio(z):
    """r = h / phi at one z <= -1"""
    from scipy.special import erfcx

    if z > SERIES_BELOW:
        t = -z / np.sqrt(2.0)
        return 1.0 - np.sqrt(np.pi) * t * erfcx(t)
    w = 1.0 / (z * z)
    s = 0.0
    for k in range(len(DOUBLE_FACTORIALS) - 1, -1, -1):
        s = s * w + (-1.0) ** k * DOUBLE_FACTORIALS[k]
    return w * s


def reference_values(mu, sd, y_max, xi, dmu=None, dsd=None):
    """logEI (n,) — and with dmu, dsd (n, d) the gradient of -logEI — point by point in fp64: the recipe as it is specified, not the
    policy's code.  sd == 0: log(aa) for aa > 0, else -inf, zero slope; NaN in, NaN out."""
    from scipy.special import ndtr

    mu = np.asarray(mu, dtype=np.float64)
    sd = np.asarray(sd, dtype=np.float64)
    n = mu.shape[0]
    val, ca, cs = np.empty(n), np.empty(n), np.empty(n)
    with np.errstate(all="ignore"):
        for i in range(n):
            aa = mu[i] - y_max - xi
            s = sd[i]
            if np.isnan(aa) or np.isnan(s):
                val[i], ca[i], cs[i] = np.nan, np.nan, np.nan
            elif s == 0.0:
                val[i], ca[i], cs[i] = (np.log(aa) if aa > 0 else -np.inf), 0.0, 0.0
            else:
                z = aa / s
                if z > -1.0:
                    Phi, phi = ndtr(z), np.exp(-(z * z) / 2.0) / np.sqrt(2.0 * np.pi)
                    h = phi + z * Phi
                    val[i], ca[i], cs[i] = np.log(s) + np.log(h), Phi / (s * h), phi / (s * h)
                else:
                    r = _ratio(z)
                    val[i] = np.log(s) + (-(z * z) / 2.0 - 0.5 * np.log(2.0 * np.pi) + np.log(r))
                    cs[i], ca[i] = 1.0 / (s * r), ((1.0 - r) / -z) / (s * r)
        if dmu is None:
            return val
        dmu = np.asarray(dmu, dtype=np.float64).reshape(n, -1)
        dsd = np.asarray(dsd, dtype=np.float64).reshape(n, -1)
        return val, -(ca[:, None] * dmu + cs[:, None] * dsd)


def argbest(neg_truth):
    """the truth's arg-best and top-k order of -logEI (mpf values; ties to the lowest index)"""
    return sorted(range(len(neg_truth)), key=lambda i: (neg_truth[i], i))
