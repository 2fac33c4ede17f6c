"""A 50-digit truth (mpmath) for the acquisition formulas, and the error model every acquisition test measures against.

The device evaluates EI / POI / the constraint factor at four sites (acq_kernel, the ACQ instances of the selection launch,
polish_fused.hip, evolve.hip).  All of them start from fp64 mu, sd and form `aa = mu - y_max - xi` left to right in fp64 with
contraction off, so the truth takes THAT fp64 value of aa as given (its rounding belongs to the subtraction, not to the formula:
a truth from the exact difference raises the reference's own constant a hundredfold) and is exact from there on:

    z = aa / sd,  EI = aa Phi(z) + sd phi(z),  POI = Phi(z)
    gradient coefficients (polish_acq_coeffs):  EI  ca = Phi, cs = phi;   POI  ca = phi / sd, cs = -phi z / sd
    constraint factor:  Phi((ub - m) / s) - Phi((lb - m) / s), lb = -inf -> 0, ub = +inf -> 1, s <= 0 -> NaN
                        (ub - m, lb - m likewise the fp64 differences)

Error model: |value - truth| <= c eps W + DBL_MIN, with the weight W = (1 + z^2) T and T the sum of the magnitudes of the terms
    EI  |aa| Phi + sd phi        POI  Phi        gradient  |ca dmu| + |cs dsd|
    factor: W = (1 + zu^2) Phi(zu) + (1 + zl^2) Phi(zl) (each end carries its own z; lb = -inf carries nothing, ub = +inf carries
    its 1: the subtraction 1 - Phi(zl) rounds at that scale).
(1 + z^2): half an ulp in the division that makes z moves ln Phi by ~ z^2 eps in the lower tail — for ANY implementation.  The
DBL_MIN floor is where fp64 itself stops holding a relative error (subnormal results); tests cap the share of points it covers.
`constants()` returns c per element with the floor taken off, so `c <= bar` IS the assertion above."""
import mpmath as mp
import numpy as np

DPS = 50
EPS = float(np.finfo(np.float64).eps)
DBL_MIN = float(np.finfo(np.float64).tiny)

_ctx = mp.mp.clone()
_ctx.dps = DPS
_SQRT2 = _ctx.sqrt(2)
_SQRT2PI = _ctx.sqrt(2 * _ctx.pi)
_NAN = _ctx.mpf("nan")


def _Phi(z):
    return _ctx.erfc(-z / _SQRT2) / 2


def _phi(z):
    return _ctx.exp(-z * z / 2) / _SQRT2PI


def _obj(values):
    out = np.empty(len(values), dtype=object)
    out[:] = values
    return out


def to_float(a):
    """mpf array -> fp64 (round to nearest; below the subnormals -> 0.0)"""
    return np.array([float(v) for v in np.ravel(a)], dtype=np.float64).reshape(np.shape(a))


def acq_truth(mu, sd, y_max, xi, dmu=None, dsd=None):
    """EI / POI truth for fp64 mu, sd (n,).  Returns a dict: `ok` (finite mu, sd and sd > 0: the truth is defined), `z` (fp64, for
    binning), `ei`, `poi` (mpf; the ACQUISITION, not its negative), `w_ei`, `w_poi` (mpf weights W), `t_ei`, `t_poi` (fp64 T).  With
    dmu, dsd (n, d) also `g_ei`, `g_poi` (mpf, = -(ca dmu + cs dsd), the gradient of -acq) and `w_g_ei`, `w_g_poi`."""
    mu = np.asarray(mu, dtype=np.float64)
    sd = np.asarray(sd, dtype=np.float64)
    n = mu.shape[0]
    aa = mu - y_max - xi                                    # the fp64 value every device site forms
    ok = np.isfinite(aa) & np.isfinite(sd) & (sd > 0)
    ei, poi, w_ei, w_poi, zs, Phis, phis = ([_NAN] * n for _ in range(7))
    for i in np.flatnonzero(ok):
        a, s = _ctx.mpf(float(aa[i])), _ctx.mpf(float(sd[i]))
        z = a / s
        P, p = _Phi(z), _phi(z)
        zs[i], Phis[i], phis[i] = z, P, p
        ei[i], poi[i] = a * P + s * p, P
        w_ei[i], w_poi[i] = (1 + z * z) * (abs(a) * P + s * p), (1 + z * z) * P
    out = {"ok": ok, "ei": _obj(ei), "poi": _obj(poi), "w_ei": _obj(w_ei), "w_poi": _obj(w_poi)}
    with np.errstate(all="ignore"):
        out["z"] = np.where(ok, aa / sd, np.nan)
    out["t_ei"] = np.array([float(w / (1 + z * z)) if o else np.nan for w, z, o in zip(w_ei, zs, ok)])
    out["t_poi"] = np.array([float(P) if o else np.nan for P, o in zip(Phis, ok)])
    if dmu is not None:
        dmu = np.asarray(dmu, dtype=np.float64).reshape(n, -1)
        dsd = np.asarray(dsd, dtype=np.float64).reshape(n, -1)
        d = dmu.shape[1]
        g = {k: np.full((n, d), _NAN, dtype=object) for k in ("g_ei", "g_poi", "w_g_ei", "w_g_poi")}
        for i in np.flatnonzero(ok & np.all(np.isfinite(dmu), axis=1) & np.all(np.isfinite(dsd), axis=1)):
            z, P, p, s = zs[i], Phis[i], phis[i], _ctx.mpf(float(sd[i]))
            for name, ca, cs in (("ei", P, p), ("poi", p / s, -p * z / s)):
                for j in range(d):
                    tm, ts = ca * _ctx.mpf(float(dmu[i, j])), cs * _ctx.mpf(float(dsd[i, j]))
                    g["g_" + name][i, j] = -(tm + ts)
                    g["w_g_" + name][i, j] = (1 + z * z) * (abs(tm) + abs(ts))
        out.update(g)
    return out


def band_truth(m, s, lb, ub):
    """The constraint factor of one constraint for fp64 posterior m, s (n,) and bounds lb, ub.  Returns `ok` (s > 0, all finite), `p`
    (mpf) and `w` (mpf weight)."""
    m = np.asarray(m, dtype=np.float64)
    s = np.asarray(s, dtype=np.float64)
    n = m.shape[0]
    lb, ub = float(lb), float(ub)
    ok = np.isfinite(m) & np.isfinite(s) & (s > 0)
    dl, du = lb - m, ub - m                                 # the fp64 differences cdf_loc_scale divides
    p, w = [_NAN] * n, [_NAN] * n
    for i in np.flatnonzero(ok):
        si = _ctx.mpf(float(s[i]))
        pl = pu = wl = wu = _ctx.mpf(0)
        if lb != -np.inf:
            zl = _ctx.mpf(float(dl[i])) / si if np.isfinite(dl[i]) else _ctx.mpf(float(dl[i]))
            pl = _Phi(zl) if np.isfinite(dl[i]) else _ctx.mpf(1 if dl[i] > 0 else 0)
            wl = (1 + zl * zl) * pl if np.isfinite(dl[i]) else _ctx.mpf(0)
        if ub != np.inf:
            zu = _ctx.mpf(float(du[i])) / si if np.isfinite(du[i]) else _ctx.mpf(float(du[i]))
            pu = _Phi(zu) if np.isfinite(du[i]) else _ctx.mpf(1 if du[i] > 0 else 0)
            wu = (1 + zu * zu) * pu if np.isfinite(du[i]) else _ctx.mpf(0)
        else:
            pu = wu = _ctx.mpf(1)                           # exactly 1, but 1 - Phi(zl) rounds at the scale of 1
        p[i], w[i] = pu - pl, wl + wu
    return {"ok": ok, "p": _obj(p), "w": _obj(w)}


def constants(got, truth, weight, floor=DBL_MIN):
    """c per element: max(0, |got - truth| - floor) / (eps W), so that `c <= bar` is `|got - truth| <= bar eps W + floor`.  inf where
    W = 0 and the error exceeds the floor; NaN where the truth is undefined (the caller compares those with the NumPy formula)."""
    got = np.asarray(got, dtype=np.float64)
    flat_t, flat_w = np.ravel(truth), np.ravel(weight)
    out = np.empty(flat_t.shape[0])
    for i, (g, t, w) in enumerate(zip(np.ravel(got), flat_t, flat_w)):
        if _ctx.isnan(t) or not np.isfinite(g):
            out[i] = np.nan if _ctx.isnan(t) else np.inf
            continue
        e = abs(_ctx.mpf(float(g)) - t) - floor
        out[i] = 0.0 if e <= 0 else (float(e / (EPS * w)) if w > 0 else np.inf)
    return out.reshape(got.shape)


# ---- the reference's own arithmetic (SciPy / NumPy), for c_ref -----------------------------------------------------------------
def reference_values(mu, sd, y_max, xi):
    """(EI, POI) as oracle.gp_oracle.base_acq computes them, with scipy.stats.norm's cdf / pdf."""
    from scipy.stats import norm

    with np.errstate(all="ignore"):
        a = mu - y_max - xi
        z = a / sd
        return a * norm.cdf(z) + sd * norm.pdf(z), norm.cdf(z)


def reference_gradients(mu, sd, dmu, dsd, y_max, xi):
    """(g_EI, g_POI) = -(ca dmu + cs dsd) in NumPy with scipy.stats.norm, as polish_acq_coeffs / polish_acq_grad spell them."""
    from scipy.stats import norm

    with np.errstate(all="ignore"):
        a = mu - y_max - xi
        z = a / sd
        cdf, pdf = norm.cdf(z), norm.pdf(z)
        g_ei = -(cdf[:, None] * dmu + pdf[:, None] * dsd)
        g_poi = -((pdf / sd)[:, None] * dmu + (-pdf * z / sd)[:, None] * dsd)
    return g_ei, g_poi


def reference_band(m, s, lb, ub):
    """One constraint's factor as oracle.gp_oracle.constraint_prob computes it."""
    from oracle.gp_oracle import _cdf_loc_scale

    p_lower = _cdf_loc_scale(lb, m, s) if lb != -np.inf else 0.0
    p_upper = _cdf_loc_scale(ub, m, s) if ub != np.inf else 1.0
    return p_upper - p_lower + np.zeros_like(m)


def worst(c):
    """the largest defined constant (0.0 if none is defined)"""
    c = np.asarray(c)[~np.isnan(c)]
    return float(c.max()) if c.size else 0.0
